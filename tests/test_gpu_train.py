"""apd_trainer on the GPU against the literal checker (tests/_train_reference.py): the weights of all four matrices, total_err, the
step count and the first non-finite step, bit for bit (NaN signs and payloads aside: _train_reference.canonical_bits) -- over the
shapes at which the kernel's loops change their trip counts (rows in blocks of 8, steps in blocks of 8, 64 lanes), over any split
of an order into runs, over models side by side, with non-finite frames, through the hand-off to the resident encoder and through
train().  The SGD is chaotic (at 2000 steps of 13 -> 8 the checker is O(1) away from its float64 twin), so only identical
arithmetic passes.  The step counts here (0, 1, 2, 63, 257) lie beside the multiples of the prefetch block: run lengths 7 .. 25 and
64, shared and per-model orders and continuations around a block edge are in tests/test_gpu_train_edges.py, with the inputs that
are not ordinary (its case table: tests/_train_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import _train_reference as ref

pytestmark = pytest.mark.gpu
F = np.float32
F32P = C.POINTER(C.c_float)
SHAPES = [(13, 8), (26, 10), (2, 1), (1, 1), (3, 2), (33, 5), (5, 33), (64, 64), (64, 1), (1, 64)]


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    yield c
    c.close()


def autoencoder(model):
    from audio_pattern_discovery_amd.neural import AutoEncoder, Mat
    d, l = model.bd.size, model.be.size
    return AutoEncoder(Mat(model.we.copy(), l), Mat(model.be.copy(), l), Mat(model.wd.copy(), d), Mat(model.bd.copy(), d))


def autoencoder_bits(nn):
    return ref.canonical_bits(np.concatenate([nn.w_encode.flat, nn.w_decode.flat, nn.b_encode.flat, nn.b_decode.flat]))


def trainer_for(ctx, models):
    from audio_pattern_discovery_amd.neural import Trainer
    return Trainer(ctx, [autoencoder(m) for m in models])


def assert_equals_checker(trainer, models, what=""):
    totals = trainer.totals()
    for m, model in enumerate(models):
        assert np.array_equal(autoencoder_bits(trainer.weights(m)), model.bits()), "%s: weights of model %d" % (what, m)
        err, steps, first = totals[m]
        assert ref.canonical_bits([err])[0] == ref.canonical_bits([model.total_err])[0], "%s: total_err of model %d" % (what, m)
        assert (steps, first) == (model.steps, model.first_nonfinite), "%s: counters of model %d" % (what, m)


def case(d, l, n_frames, seed, sd=2.0):
    rng = np.random.default_rng(seed)
    return rng, ref.seeded(rng, d, l), (rng.standard_normal((n_frames, d)) * sd).astype(F)


@pytest.mark.parametrize("d,l", SHAPES)
def test_every_shape_and_step_count_is_the_checkers_bits(ctx, d, l):
    """0, 1, 2, 63 and 257 steps of one order (repeated indices; frames 90 .. 99 are never touched) from the same start.  D = 1 turns
    NaN at step 0, as in the reference."""
    rng, start, frames = case(d, l, 100, 7000 + 100 * d + l)
    order = rng.integers(0, 90, 257).astype(np.uint32)
    model, at = start.copy(), 0
    for steps in (0, 1, 2, 63, 257):
        model.run(frames, order[at:steps], 0.1)
        at = steps
        with trainer_for(ctx, [start]) as t:
            t.run(frames, order[:steps], 0.1)
            assert_equals_checker(t, [model], "%d -> %d, %d steps" % (d, l, steps))
    assert (model.first_nonfinite == 0) == (d == 1)


def test_2000_steps_at_13_to_8(ctx):
    rng, model, frames = case(13, 8, 500, 42)
    order = rng.integers(0, 500, 2000).astype(np.uint32)
    with trainer_for(ctx, [model]) as t:
        t.run(frames, order, 0.1)
        model.run(frames, order, 0.1)
        assert model.first_nonfinite is None
        assert_equals_checker(t, [model], "2000 steps")


def test_frames_on_the_device_one_float_off_a_16_byte_boundary(ctx):
    rng, model, frames = case(13, 8, 64, 43)
    order = rng.integers(0, 64, 100).astype(np.uint32)
    buf = ctx.alloc(frames.nbytes + 16)
    buf.copy_from(frames, 4)
    with trainer_for(ctx, [model]) as t:
        t.run((buf.at(4), 64), order, 0.05, on_device=True)
        model.run(frames, order, 0.05)
        assert_equals_checker(t, [model], "device frames")
    buf.free()


def test_any_split_of_an_order_leaves_the_bits_of_one_run(ctx):
    """257 steps at once; as 1 + 0 + 63 + 193; as 257 runs of one step; as 257 calls of AutoEncoder.take_step; and with a
    totals(reset=True) in the middle, which changes total_err and steps only."""
    rng, model, frames = case(13, 8, 80, 44)
    order = rng.integers(0, 80, 257).astype(np.uint32)
    with trainer_for(ctx, [model]) as whole, trainer_for(ctx, [model]) as parts, trainer_for(ctx, [model]) as single, \
            trainer_for(ctx, [model]) as reset:
        whole.run(frames, order, 0.1)
        at = 0
        for n in (1, 0, 63, 193):
            parts.run(frames, order[at:at + n], 0.1)
            at += n
        for i in order:
            single.run(frames, [i], 0.1)
        reset.run(frames, order[:100], 0.1)
        head = reset.totals(reset=True)[0]
        reset.run(frames, order[100:], 0.1)
        nn = autoencoder(model)
        errors = [nn.take_step(frames[i], 0.1, ctx) for i in order]
        half = model.copy().run(frames, order[:100], 0.1)
        tail = half.copy()
        tail.reset_totals()
        tail.run(frames, order[100:], 0.1)
        model.run(frames, order, 0.1)
        for t, name in ((whole, "one run"), (parts, "1 + 0 + 63 + 193"), (single, "257 runs")):
            assert_equals_checker(t, [model], name)
        assert np.array_equal(autoencoder_bits(nn), model.bits())
        total = F(0.0)
        for e in errors:
            total = total + F(e)
        assert total == model.total_err
        assert ref.canonical_bits([head[0]])[0] == ref.canonical_bits([half.total_err])[0] and head[1:] == (100, None)
        assert_equals_checker(reset, [tail], "reset in the middle")                 # steps 157, total_err of the tail, weights of the whole
        assert np.array_equal(tail.bits(), model.bits())


def test_models_side_by_side_are_the_models_alone(ctx):
    """8 models with their own inits, learning rates and orders: each equals the checker and itself trained alone.  8 equal inits with
    a shared order: all bit-equal.  Two identical calls on fresh trainers: identical bytes."""
    rng = np.random.default_rng(45)
    models = [ref.seeded(rng, 13, 8) for _ in range(8)]
    frames = (rng.standard_normal((120, 13)) * 2.0).astype(F)
    orders = rng.integers(0, 120, (8, 150)).astype(np.uint32)
    alphas = np.linspace(0.02, 0.16, 8).astype(F)
    images = []
    for rep in range(2):
        with trainer_for(ctx, models) as t:
            t.run(frames, orders, alphas)
            images.append(np.concatenate([autoencoder_bits(t.weights(m)) for m in range(8)]).tobytes() + repr(t.totals()).encode())
            if rep == 0:
                alone = []
                for m in range(8):
                    with trainer_for(ctx, [models[m]]) as one:
                        one.run(frames, orders[m], alphas[m])
                        alone.append((autoencoder_bits(one.weights(0)).tobytes(), one.totals()[0]))
                    assert alone[m][0] == autoencoder_bits(t.weights(m)).tobytes() and repr(alone[m][1]) == repr(t.totals()[m])
                trained = [models[m].copy().run(frames, orders[m], alphas[m]) for m in range(8)]
                assert_equals_checker(t, trained, "8 models")
    assert images[0] == images[1]
    with trainer_for(ctx, [models[3]] * 8) as t:
        t.run(frames, orders[0], 0.1)
        same = models[3].copy().run(frames, orders[0], 0.1)
        assert_equals_checker(t, [same] * 8, "8 equal models")


@pytest.mark.parametrize("kind", ["nan", "inf", "-inf", "constant", "inf and constant rest"])
def test_a_non_finite_or_constant_frame_at_step_100(ctx, kind):
    """The middle one of three models meets the frame at step 100 of 257; its neighbours, on an order that avoids it, stay as they
    would alone.  A NaN, an infinity and a constant frame (0 / 0 in Mat::norm) each leave NaN weights from that step on."""
    rng = np.random.default_rng(46)
    models = [ref.seeded(rng, 13, 8) for _ in range(3)]
    frames = (rng.standard_normal((60, 13)) * 2.0).astype(F)
    if kind == "constant":
        frames[59] = 1.25
    elif kind == "inf and constant rest":
        frames[59] = 3.0
        frames[59, 0] = np.inf
    else:
        frames[59, 4] = {"nan": np.nan, "inf": np.inf, "-inf": -np.inf}[kind]
    orders = rng.integers(0, 59, (3, 257)).astype(np.uint32)
    orders[1, 100] = 59
    with trainer_for(ctx, models) as t:
        t.run(frames, orders, 0.1)
        trained = [models[m].copy().run(frames, orders[m], 0.1) for m in range(3)]
        assert trained[1].first_nonfinite == 100 and trained[0].first_nonfinite is None and trained[2].first_nonfinite is None
        assert np.isnan(trained[1].we).all() and np.isnan(trained[1].total_err)
        assert_equals_checker(t, trained, kind)


def test_hand_off_to_the_resident_encoder_and_the_file_format(ctx, apd):
    from audio_pattern_discovery_amd.neural import AutoEncoder
    rng, model, frames = case(13, 8, 200, 47)
    order = rng.integers(0, 200, 300).astype(np.uint32)
    with trainer_for(ctx, [ref.seeded(rng, 13, 8), model]) as t:
        t.run(frames, order, 0.1)
        nn = t.weights(1)
        enc = t.encoder(1)
        t.run(frames, order, 0.1)                                        # the encoder owns a copy: later steps do not reach it
    d_x, d_out = ctx.upload(frames), ctx.alloc(200 * 8 * 4)              # the trainer is gone, the encoder lives
    enc.encode_async(d_x.at(), 200, d_out.at())
    ctx.synchronize()
    got = d_out.to_numpy(F)
    assert np.array_equal(got.view(np.uint32), nn.predict_frames(frames, ctx).ravel().view(np.uint32))
    enc.close()
    back = AutoEncoder.from_bytes(nn.to_bytes())
    assert np.array_equal(autoencoder_bits(back), autoencoder_bits(nn)) and back.to_bytes() == nn.to_bytes()
    assert np.array_equal(autoencoder_bits(nn), model.copy().run(frames, order, 0.1).bits())


def test_train_equals_the_checkers_replay_of_the_reference_loop(ctx):
    from audio_pattern_discovery_amd.discovery import Discovery
    from audio_pattern_discovery_amd.neural import train
    rng = np.random.default_rng(48)
    offsets = np.array([0, 5, 45, 57, 80], np.uint64)                    # 4 ragged signals of 5 .. 40 frames
    frames = (rng.standard_normal((80, 13)) * 2.0).astype(F)
    cfg = Discovery(auto_encoder=8, epochs=3, epoch_drop=2.0, learning_rate=0.1, drop=0.5)
    models = [ref.seeded(rng, 13, 8) for _ in range(2)]
    trained, means = train(frames, offsets, cfg, [autoencoder(m) for m in models], seed=9, ctx=ctx)
    want = ref.train_loop(frames, offsets, cfg, models, 9)
    assert means.shape == (3, 2) and np.array_equal(means.view(np.uint32), want.view(np.uint32))
    for nn, model in zip(trained, models):
        assert np.array_equal(autoencoder_bits(nn), model.bits())
    fresh, _ = train(frames, offsets, cfg, 2, seed=9, ctx=ctx)           # models by number: AutoEncoder.new from default_rng(seed + m)
    again, _ = train(frames, offsets, cfg, 2, seed=9, ctx=ctx)
    assert [autoencoder_bits(a).tobytes() for a in fresh] == [autoencoder_bits(a).tobytes() for a in again]
    assert fresh[0].w_encode.rows() == 13 and fresh[0].n_latent() == 8


def test_limits_and_errors(ctx, apd):
    from audio_pattern_discovery_amd.neural import Trainer
    L = apd.lib()
    rng = np.random.default_rng(49)
    for d, l in ((65, 8), (8, 65)):
        with pytest.raises(apd.ApdError) as e:
            trainer_for(ctx, [ref.seeded(rng, d, l)])
        assert e.value.status == apd.APD_ERR_UNSUPPORTED
    model = ref.seeded(rng, 3, 2)
    frames = rng.standard_normal((10, 3)).astype(F)
    with trainer_for(ctx, [model]) as t:
        t.run(frames, [1, 2, 3], 0.1)
        before = (autoencoder_bits(t.weights(0)).tobytes(), repr(t.totals()))
        with pytest.raises(apd.ApdError) as e:
            t.run(frames, [4, 10, 5], 0.1)                               # index n_frames
        assert e.value.status == apd.APD_ERR_INVALID_ARG
        assert (autoencoder_bits(t.weights(0)).tobytes(), repr(t.totals())) == before
        other = apd.Context(0)
        a = np.zeros(1, F)
        o = np.zeros(1, np.uint32)
        bad = apd.APD_ERR_INVALID_ARG
        assert L.apd_trainer_run(other.handle, t.handle, C.c_void_p(frames.ctypes.data), 10, 0, o.ctypes.data_as(C.POINTER(C.c_uint32)), 1, 0,
                                 a.ctypes.data_as(F32P)) == bad
        enc = C.c_void_p()
        assert L.apd_trainer_encoder(other.handle, t.handle, 0, C.byref(enc)) == bad
        assert L.apd_trainer_encoder(ctx.handle, t.handle, 1, C.byref(enc)) == bad
        assert L.apd_trainer_run(ctx.handle, t.handle, None, 10, 0, o.ctypes.data_as(C.POINTER(C.c_uint32)), 1, 0, a.ctypes.data_as(F32P)) == bad
        assert L.apd_trainer_run(ctx.handle, t.handle, C.c_void_p(frames.ctypes.data), 10, 0, None, 1, 0, a.ctypes.data_as(F32P)) == bad
        assert L.apd_trainer_run(ctx.handle, t.handle, C.c_void_p(frames.ctypes.data), 10, 0, o.ctypes.data_as(C.POINTER(C.c_uint32)), 1, 0, None) == bad
        assert L.apd_trainer_weights(t.handle, 1, a.ctypes.data_as(F32P), a.ctypes.data_as(F32P), a.ctypes.data_as(F32P), a.ctypes.data_as(F32P)) == bad
        other.close()
        assert (autoencoder_bits(t.weights(0)).tobytes(), repr(t.totals())) == before
    w = np.zeros(6, F)
    h = C.c_void_p()
    p = w.ctypes.data_as(F32P)
    assert L.apd_trainer_create(ctx.handle, 3, 2, 0, p, p, p, p, C.byref(h)) == apd.APD_ERR_INVALID_ARG
    assert L.apd_trainer_create(ctx.handle, 3, 2, 1, p, None, p, p, C.byref(h)) == apd.APD_ERR_INVALID_ARG
    assert L.apd_trainer_create(None, 3, 2, 1, p, p, p, p, C.byref(h)) == apd.APD_ERR_INVALID_ARG
    assert L.apd_trainer_totals(None, None, None, None, 0) == apd.APD_ERR_INVALID_ARG
    with pytest.raises(apd.ApdError):
        Trainer(ctx, [])
    # a trainer destroyed while its encoder lives, and both outliving their context
    own = apd.Context(0)
    t = trainer_for(own, [model])
    enc = t.encoder(0)
    t.close()
    d_x, d_out = own.upload(frames), own.alloc(10 * 2 * 4)
    enc.encode_async(d_x.at(), 10, d_out.at())
    own.synchronize()
    assert np.array_equal(d_out.to_numpy(F).view(np.uint32), autoencoder(model).predict_frames(frames, own).ravel().view(np.uint32))
    t2 = trainer_for(own, [model])
    d_x.free()
    d_out.free()
    own.close()
    t2.close()
    enc.close()
