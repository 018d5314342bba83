"""apd_trainer_evaluate on the GPU against its checker (tests/_train_eval_reference.py): per-frame errors, the sequential totals and
the first non-finite position, bit for bit (canonical_bits) -- over the shapes and lengths at which the kernels' loops and tiles
change, every form of order and placement, frames and models that are not finite, the chunked call, many models, and the existing
training kernel at a rate of zero as a second device implementation of the same sum.  And that nothing of the trainer moves."""
import ctypes as C

import numpy as np
import pytest

import _train_cases as cases
import _train_eval_reference as ev
import _train_reference as ref

pytestmark = pytest.mark.gpu
F = np.float32
SHAPES = [(1, 1), (2, 1), (3, 2), (13, 8), (26, 10), (5, 33), (33, 5), (64, 1), (1, 64), (64, 64)]
# positions per workgroup of train_eval_kernel are 256, 128 or 64 by shape (csrc/train.hip, eval_tile): every one of them +- 1
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257)
# the share of the sigmoid probe's finite arguments that the lemma of _train_eval_reference makes fully observed: computed from the
# checker alone by tests/test_train_eval_reference.py::test_probe_lemma (0.9094), asserted here as a floor
PROBE_OBSERVED_FLOOR = 0.9094


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    yield c
    c.close()


def autoencoder(model):
    from audio_pattern_discovery_amd.neural import AutoEncoder, Mat
    d, l = model.bd.size, model.be.size
    return AutoEncoder(Mat(model.we.copy(), l), Mat(model.be.copy(), l), Mat(model.wd.copy(), d), Mat(model.bd.copy(), d))


def as_model(nn):
    return ref.Model(nn.w_encode.flat, nn.w_decode.flat, nn.b_encode.flat, nn.b_decode.flat)


def trainer_for(ctx, models):
    from audio_pattern_discovery_amd.neural import Trainer
    return Trainer(ctx, [autoencoder(m) for m in models])


def bits(a):
    return ref.canonical_bits(np.asarray(a, F))


def state_bits(t):
    """Everything the trainer holds that a caller can read: weights of every model, totals, steps, first non-finite step."""
    w = np.concatenate([np.concatenate([a.flat for a in (nn.w_encode, nn.w_decode, nn.b_encode, nn.b_decode)]) for nn in map(t.weights, range(t.n_models))])
    totals = t.totals()
    return bits(w).tobytes(), bits([e for e, _, _ in totals]).tobytes(), [(s, f) for _, s, f in totals]


def assert_equals_checker(got, models, frames, order=None, what=""):
    errors, totals, firsts = got
    want = ev.evaluate_many(models, frames, order)
    assert errors.shape == want[0].shape, what
    for m in range(len(models)):
        assert np.array_equal(bits(errors[m]), bits(want[0][m])), "%s: errors of model %d" % (what, m)
    assert np.array_equal(bits(totals), bits(want[1])), "%s: totals" % what
    assert list(firsts) == want[2], "%s: first non-finite positions" % what


def case(d, l, n_models, n_frames, seed, sd=2.0):
    rng = np.random.default_rng(seed)
    models = [ref.seeded(np.random.default_rng(seed + 1 + m), d, l) for m in range(n_models)]
    return rng, models, (rng.standard_normal((n_frames, d)) * sd).astype(F)


# ---- shapes x lengths
@pytest.mark.parametrize("d,l", SHAPES)
def test_every_shape_and_length_is_the_checkers_bits(ctx, d, l):
    """3 models with their own seeds, a shared order with repeats, every length of LENGTHS.  At 1 -> 1 and 1 -> 64 every frame is
    constant: every error is NaN and the first non-finite position is 0."""
    rng, models, frames = case(d, l, 3, 100, 11000 + 100 * d + l)
    order = rng.integers(0, 100, max(LENGTHS)).astype(np.uint32)
    with trainer_for(ctx, models) as t:
        for n in LENGTHS:
            got = t.evaluate(frames, order[:n], errors=True)
            assert_equals_checker(got, models, frames, order[:n], "%d -> %d, %d positions" % (d, l, n))
            if d == 1 and n:
                assert np.isnan(got[0]).all() and got[2] == [0, 0, 0]
            if n == 0:
                assert got[0].shape == (3, 0) and bits(got[1]).tolist() == [0, 0, 0] and got[2] == [None] * 3


# ---- orders
def test_orders_null_shared_reversed_last_and_per_model(ctx):
    rng, models, frames = case(13, 8, 3, 77, 12000)
    with trainer_for(ctx, models) as t:
        assert_equals_checker(t.evaluate(frames, errors=True), models, frames, None, "order NULL")
        for name, order in (("repeats", rng.integers(0, 77, 131)), ("reversed", np.arange(77)[::-1]), ("all the last frame", np.full(70, 76))):
            assert_equals_checker(t.evaluate(frames, order.astype(np.uint32), errors=True), models, frames, order, name)
        for n in (67, 131):                                            # rows start 67 and 131 entries apart: no multiple of 8 or 64
            order = rng.integers(0, 77, (3, n)).astype(np.uint32)
            order[:, -1] = 76
            assert_equals_checker(t.evaluate(frames, order, errors=True), models, frames, order, "per model, %d positions" % n)


def test_an_index_equal_to_n_frames_is_refused_and_nothing_moves(ctx, apd):
    rng, models, frames = case(13, 8, 3, 40, 12100)
    with trainer_for(ctx, models) as t:
        t.run(frames, rng.integers(0, 40, 20).astype(np.uint32), 0.1)
        before = state_bits(t)
        for order in (np.array([0, 1, 40], np.uint32), np.array([[0, 1, 2], [3, 4, 5], [6, 7, 40]], np.uint32)):
            with pytest.raises(apd.ApdError) as e:
                t.evaluate(frames, order)
            assert e.value.status == apd.APD_ERR_INVALID_ARG
            assert b"apd_trainer_evaluate" in apd.lib().apd_last_error(ctx.handle)
        assert state_bits(t) == before


# ---- placement
def test_device_frames_and_device_errors_one_float_off_a_16_byte_boundary(ctx):
    rng, models, frames = case(13, 8, 3, 64, 12200)
    order = rng.integers(0, 64, 150).astype(np.uint32)
    d_frames = ctx.alloc(frames.nbytes + 16)
    d_frames.copy_from(frames, 4)
    d_err = ctx.alloc(3 * 150 * 4 + 16)
    d_err.fill(0xFF)
    with trainer_for(ctx, models) as t:
        host = t.evaluate(frames, order, errors=True)
        _, totals, firsts = t.evaluate((d_frames.at(4), 64), order, on_device=True, errors=d_err.at(4))
        device_errors = d_err.to_numpy(F, 3 * 150, 4).reshape(3, 150)
        assert np.array_equal(d_err.to_numpy(np.uint32, 1), [0xFFFFFFFF])          # the float in front is not written
        assert_equals_checker((device_errors, totals, firsts), models, frames, order, "device frames and errors")
        assert np.array_equal(bits(host[0]), bits(device_errors)) and np.array_equal(bits(host[1]), bits(totals)) and host[2] == firsts
    d_frames.free()
    d_err.free()


# ---- special frames
def special_frames(d):
    norm = cases.norm_frames(d)
    named = {"constant": np.full(d, 0.25, F), "nan": np.resize(np.array([1.0, np.nan, 2.0], F), d), "+inf": np.resize(np.array([np.inf, 0.5, -1.0], F), d),
             "-inf": np.resize(np.array([0.5, -np.inf, -1.0], F), d)}
    for name in ("spread below 1e-8", "spread just under 1e-8", "spread exactly 1e-8", "inf and a spread below 1e-8"):
        named[name] = norm[name][0]
    return named


@pytest.mark.parametrize("d,l", [(13, 8), (64, 7)])
def test_special_frames_cost_their_own_positions_only(ctx, d, l):
    """One model per special frame, which meets it at positions 0, 64 and the last of 130 (a per-model order).  Every error is the
    checker's; the other positions have the bits of a call without the special frames; the weights stay finite and unchanged.  The
    same orders through run(alpha = 0) on a second trainer: a constant, NaN or infinite frame turns that model non-finite at step 0."""
    special = special_frames(d)
    rng, models, plain = case(d, l, len(special), 50, 12300 + d)
    frames = np.concatenate([plain, np.stack(list(special.values()))])
    base = rng.integers(0, 50, 130).astype(np.uint32)
    order = np.tile(base, (len(special), 1))
    at = [0, 64, 129]
    for m in range(len(special)):
        order[m, at] = 50 + m
    with trainer_for(ctx, models) as t, trainer_for(ctx, models) as clone:
        before = state_bits(t)
        got = t.evaluate(frames, order, errors=True)
        assert_equals_checker(got, models, frames, order, "special frames")
        without = t.evaluate(frames, base, errors=True)
        others = np.setdiff1d(np.arange(130), at)
        assert np.array_equal(bits(got[0][:, others]), bits(without[0][:, others]))
        assert np.isfinite(without[0]).all() and without[2] == [None] * len(special)
        for m, name in enumerate(special):
            poisons = name in ("constant", "nan", "+inf", "-inf", "inf and a spread below 1e-8")
            assert (got[2][m] == 0) == poisons and (not np.isfinite(got[1][m])) == poisons, name
            assert np.isfinite(got[0][m, others]).all(), name
        assert state_bits(t) == before and all(as_model(t.weights(m)).finite() for m in range(len(special)))
        clone.run(frames, order, 0.0)
        for m, (name, (_, _, first)) in enumerate(zip(special, clone.totals())):
            want = models[m].copy().run(frames, order[m], 0.0)
            assert first == want.first_nonfinite, name
            if name in ("constant", "nan", "+inf", "-inf"):
                assert first == 0 and not as_model(clone.weights(m)).finite(), name


# ---- models that are not finite
def test_a_non_finite_model_leaves_its_neighbours_alone(ctx):
    rng, models, frames = case(13, 8, 5, 60, 12400)
    models[1].wd[3, 4] = np.inf
    models[3].we[7, 2] = np.nan
    order = rng.integers(0, 60, 100).astype(np.uint32)
    with trainer_for(ctx, models) as t, trainer_for(ctx, [models[0], models[2], models[4]]) as finite:
        got = t.evaluate(frames, order, errors=True)
        assert_equals_checker(got, models, frames, order, "inf and NaN weights")
        # the NaN weight reaches every error of its model; the +inf one only saturates a sigmoid (output 4 is +-inf, act 4 is 0 or 1)
        assert got[2][3] == 0 and got[2][0] is got[2][1] is got[2][2] is got[2][4] is None and np.isfinite(got[0][1]).all()
        alone = finite.evaluate(frames, order, errors=True)
        assert np.array_equal(bits(got[0][[0, 2, 4]]), bits(alone[0])) and np.array_equal(bits(got[1][[0, 2, 4]]), bits(alone[1]))


# ---- the defined sigmoid, through the probe of _train_eval_reference
def test_sigmoid_through_the_probe(ctx):
    """error = 0.5 * sigmoid(u) exactly wherever sigmoid(u)^2 is normal: the device's error then carries every bit of its sigmoid.  64
    models per launch, one argument per model, three positions of the probe frame."""
    args, n = ev.probe_arguments()
    flat = args.ravel()
    got = np.empty((flat.size, 3), F)
    for k, launch in enumerate(args):
        with trainer_for(ctx, [ev.probe_model(u) for u in launch]) as t:
            got[k * 64:(k + 1) * 64] = t.evaluate(ev.PROBE_FRAME, np.zeros(3, np.uint32), errors=True)[0]
    want = np.array([ev.error_of(ev.probe_model(u), ev.PROBE_FRAME[0]) for u in flat], F)
    for p in range(3):
        assert np.array_equal(bits(got[:, p]), bits(want))             # every argument, observed or not
    with np.errstate(all="ignore"):
        half_sigmoid = (F(0.5) * ref.sigmoid_defined(flat)).astype(F)
    observed = bits(got[:n, 0]) == bits(half_sigmoid[:n])
    finite = np.isfinite(flat[:n])
    assert observed[finite].mean() >= PROBE_OBSERVED_FLOOR
    assert observed[~finite].all()                                     # +inf -> 0.5, -inf -> 0, NaN -> NaN


# ---- the state is untouched
def test_evaluate_between_runs_leaves_the_bits_of_one_run(ctx):
    rng, models, frames = case(13, 8, 3, 80, 12500)
    order = rng.integers(0, 80, 257).astype(np.uint32)
    held_out = (rng.standard_normal((90, 13)) * 2.0).astype(F)
    held_out[17] = 1.5                                                 # a constant frame among them
    with trainer_for(ctx, models) as whole, trainer_for(ctx, models) as parts:
        whole.run(frames, order, 0.1)
        parts.run(frames, order[:100], 0.1)
        encoder_before = parts.encoder(1)
        mid = state_bits(parts)
        first = parts.evaluate(held_out, errors=True)
        second = parts.evaluate(held_out, errors=True)
        assert state_bits(parts) == mid
        assert np.array_equal(bits(first[0]), bits(second[0])) and np.array_equal(bits(first[1]), bits(second[1])) and first[2] == second[2] == [17] * 3
        assert_equals_checker(first, [as_model(parts.weights(m)) for m in range(3)], held_out, None, "after 100 steps")
        # the encoder of after the evaluation encodes as the one of before
        encoder_after = parts.encoder(1)
        x, outs = ctx.upload(held_out[:16]), []
        for enc in (encoder_before, encoder_after):
            out = ctx.alloc(16 * 8 * 4)
            enc.encode_async(x.at(), 16, out.at())
            ctx.synchronize()
            outs.append(out.to_numpy(F))
            out.free()
            enc.close()
        x.free()
        assert np.array_equal(bits(outs[0]), bits(outs[1]))
        parts.run(frames, order[100:], 0.1)
        assert state_bits(parts) == state_bits(whole)


# ---- against the existing kernel: two device implementations of one sum
@pytest.mark.parametrize("d,l", [(13, 8), (64, 64)])
def test_totals_are_those_of_the_training_kernel_at_rate_zero(ctx, d, l):
    rng, models, frames = case(d, l, 3, 120, 12600 + d)
    for order in (rng.integers(0, 120, 300).astype(np.uint32), rng.integers(0, 120, (3, 300)).astype(np.uint32)):
        with trainer_for(ctx, models) as t, trainer_for(ctx, models) as clone:
            totals, firsts = t.evaluate(frames, order)
            clone.run(frames, order, 0.0)
            ran = clone.totals()
            assert np.array_equal(bits(totals), bits([e for e, _, _ in ran])) and firsts == [None] * 3
            assert all(s == 300 and f is None for _, s, f in ran) and np.isfinite(totals).all()


# ---- chunking
@pytest.mark.parametrize("cap,chunk", [(5 * 4 * 100, 100), (5 * 4, 1), (5 * 4 * 257, 257)])
def test_chunked_calls_give_the_bits_of_the_uncut_call(ctx, monkeypatch, cap, chunk):
    """APD_EVAL_WORKSPACE_BYTES is read at every call.  5 models x 257 positions cut every 100 positions (no multiple of 64), every
    position, and not at all; a constant frame at position 150 for model 2 only, so its first non-finite position lies across a cut."""
    rng, models, frames = case(13, 8, 5, 60, 12700)
    frames[59] = -2.0
    order = rng.integers(0, 59, (5, 257)).astype(np.uint32)
    order[2, 150] = 59
    d_err = ctx.alloc(5 * 257 * 4)
    with trainer_for(ctx, models) as t:
        uncut = t.evaluate(frames, order, errors=True)
        assert uncut[2] == [None, None, 150, None, None]
        monkeypatch.setenv("APD_EVAL_WORKSPACE_BYTES", str(cap))
        cut = t.evaluate(frames, order, errors=True)
        _, totals, firsts = t.evaluate(frames, order, errors=d_err.at())
        monkeypatch.delenv("APD_EVAL_WORKSPACE_BYTES")
        for errors, tot, fst in (cut, (d_err.to_numpy(F).reshape(5, 257), totals, firsts)):
            assert np.array_equal(bits(errors), bits(uncut[0])) and np.array_equal(bits(tot), bits(uncut[1])) and fst == uncut[2], chunk
        assert_equals_checker(cut, models, frames, order, "cut every %d" % chunk)
    d_err.free()


# ---- many models
@pytest.mark.parametrize("d,l,n_models", [(3, 2, 1500), (64, 64, 300)])
def test_many_models(ctx, d, l, n_models):
    rng, models, frames = case(d, l, n_models, 65, 12800 + d)
    with trainer_for(ctx, models) as t:
        got = t.evaluate(frames, errors=True)
        assert_equals_checker(got, models, frames, None, "%d models" % n_models)
        for m in (0, n_models // 2, n_models - 1):
            with trainer_for(ctx, [models[m]]) as alone:
                one = alone.evaluate(frames, errors=True)
                assert np.array_equal(bits(one[0][0]), bits(got[0][m])) and bits(one[1])[0] == bits(got[1][m:m + 1])[0]


# ---- after training
def test_picking_the_best_of_eight_trained_models(ctx):
    rng, models, frames = case(13, 8, 8, 300, 12900)
    held_out = (rng.standard_normal((150, 13)) * 2.0).astype(F)
    order = rng.integers(0, 300, 200).astype(np.uint32)
    rates = np.array([0.3, 0.2, 0.1, 0.05, 0.02, 0.01, 0.003, 0.0], F)
    with trainer_for(ctx, models) as t:
        t.run(frames, order, rates)
        got = t.evaluate(held_out, errors=True)
        trained = [as_model(t.weights(m)) for m in range(8)]
        assert_equals_checker(got, trained, held_out, None, "trained models")
        want = ev.evaluate_many(trained, held_out)[1]
        best, totals = t.best(held_out)
        assert best == int(np.argmin(want)) and np.array_equal(bits(totals), bits(want)) and np.isfinite(want).all()
        one = t.weights(best).reconstruction_errors(held_out, ctx)
        assert np.array_equal(bits(one), bits(got[0][best]))


# ---- refusals
def test_refusals_name_the_call(ctx, apd):
    rng, models, frames = case(13, 8, 2, 10, 13000)
    L = apd.lib()
    other = apd.Context(0)
    u32p, f32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    order = np.arange(10, dtype=np.uint32)
    total, first = np.zeros(2, F), np.zeros(2, np.uint64)
    x, o, tp, fp = C.c_void_p(frames.ctypes.data), order.ctypes.data_as(u32p), total.ctypes.data_as(f32p), first.ctypes.data_as(u64p)
    with trainer_for(ctx, models) as t:
        before = state_bits(t)
        h = t.handle
        calls = {
            "a trainer of another context": (other.handle, (other.handle, h, x, 10, 0, o, 10, 0, None, 0, tp, fp)),
            "NULL frames": (ctx.handle, (ctx.handle, h, None, 10, 0, o, 10, 0, None, 0, tp, fp)),
            "all outputs NULL": (ctx.handle, (ctx.handle, h, x, 10, 0, o, 10, 0, None, 0, None, None)),
            "order NULL, n_eval != n_frames": (ctx.handle, (ctx.handle, h, x, 10, 0, None, 9, 0, None, 0, tp, fp)),
            "order_per_model with a NULL order": (ctx.handle, (ctx.handle, h, x, 10, 0, None, 10, 1, None, 0, tp, fp)),
            "2^32 frames": (ctx.handle, (ctx.handle, h, x, 1 << 32, 0, o, 10, 0, None, 0, tp, fp)),
        }
        messages = set()
        for name, (owner, args) in calls.items():
            assert L.apd_trainer_evaluate(*args) == apd.APD_ERR_INVALID_ARG, name
            assert b"apd_trainer_evaluate" in L.apd_last_error(owner), name
            messages.add(L.apd_last_error(owner))
        assert len(messages) == len(calls)                             # every refusal wrote its own reason
        assert L.apd_trainer_evaluate(ctx.handle, None, x, 10, 0, o, 10, 0, None, 0, tp, fp) == apd.APD_ERR_INVALID_ARG
        assert L.apd_trainer_evaluate(ctx.handle, h, x, 10, 0, o, 10, 0, None, 0, tp, fp) == apd.APD_OK     # and the same call, whole
        assert state_bits(t) == before
    other.close()


def test_timing_covers_the_evaluation(ctx):
    rng, models, frames = case(13, 8, 2, 500, 13100)
    with trainer_for(ctx, models) as t:
        ctx.set_timing(True)
        t.evaluate(frames)
        ms = ctx.last_kernel_ms()
        ctx.set_timing(False)
        assert 0.0 < ms < 1000.0
