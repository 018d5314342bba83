"""CPU tests of the trainer's definition: the checker of tests/_train_reference.py against its float64 twin on
short horizons (where such a comparison means something: the SGD is chaotic), the defined exponential against the true one, answers
worked out by hand, apd_train_order / apd_step_decay against the checker's generator, and the single-thread C++ restatement
(tools/train_cpu.cpp, built with the library's host-only unit under AddressSanitizer + UBSan and run as a program) against the
checker's bits.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _train_reference as ref

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("d,l,sd", [(13, 8, 2.0), (13, 8, 0.5), (3, 2, 2.0)])
def test_checker_stays_with_its_float64_twin_for_400_steps(d, l, sd):
    """400 steps at lr 0.1 on frames ~ N(0, sd^2) from Mat::seeded weights: the largest weight difference between the f32 checker
    (defined sigmoid) and the float64 twin (true exp) stays under 1e-4.  The same checker with numpy's f32 exp is printed beside it."""
    rng = np.random.default_rng(1000 + d * 10 + int(sd * 10))
    model = ref.seeded(rng, d, l)
    twin = ref.Model(model.we, model.wd, model.be, model.bd, np.float64)
    libm = ref.Model(model.we, model.wd, model.be, model.bd, F, ref.sigmoid_libm)
    frames = (rng.standard_normal((400, d)) * sd).astype(F)
    for x in frames:
        model.step(x, 0.1)
        twin.step(x.astype(np.float64), np.float64(F(0.1)))
        libm.step(x, 0.1)
    mine, theirs = ref.max_weight_difference(model, twin), ref.max_weight_difference(libm, twin)
    print("(%d, %d, sd %.1f): defined sigmoid %.3e, numpy expf %.3e from the float64 twin" % (d, l, sd, mine, theirs))
    assert model.first_nonfinite is None and twin.finite()
    assert mine < 1e-4


def test_defined_exp_is_within_two_ulp_of_exp():
    """Every f32 whose low 8 mantissa bits are zero (2^24 patterns), wherever exp of it is a normal f32: at most 2 ulp from the
    float64 exp.  Measured: 0.97."""
    bits = np.arange(1 << 24, dtype=np.uint32) << np.uint32(8)
    worst, checked = 0.0, 0
    for chunk in np.array_split(bits, 16):
        t = chunk.view(F)
        t = t[np.isfinite(t)]
        with np.errstate(over="ignore"):
            exact = np.exp(t.astype(np.float64))
        normal = (exact >= float(np.finfo(F).tiny)) & (exact <= float(np.finfo(F).max))
        t, exact = t[normal], exact[normal]
        if not t.size:
            continue
        got = ref.exp_defined(t).astype(np.float64)
        ulp = np.spacing(exact.astype(F)).astype(np.float64)
        worst = max(worst, float(np.max(np.abs(got - exact) / ulp)))
        checked += t.size
    print("defined exp: %d arguments, worst %.3f ulp" % (checked, worst))
    assert checked > 8_000_000                  # both signs, every exponent up to |t| ~ 88 (the larger ones overflow or underflow)
    assert worst <= 2.0


def test_sigmoid_saturation_nan_and_infinities():
    one = ref.sigmoid_defined(np.array([17.4, 20.0, 50.0, 88.0, 104.0, 105.0, 200.0, 1e30, np.inf], F))
    assert np.array_equal(one.view(np.uint32), np.full(9, F(1.0)).view(np.uint32))
    zero = ref.sigmoid_defined(np.array([-89.0, -100.0, -104.0, -105.0, -200.0, -1e30, -np.inf], F))
    assert np.array_equal(zero.view(np.uint32), np.zeros(7, np.uint32))            # +0.0 exactly: 1 / (1 + inf)
    edge = ref.sigmoid_defined(np.array([-88.0, -87.0, 16.0, 0.0], F))
    assert 0.0 < edge[0] < edge[1] < 1e-37 and edge[2] < 1.0 and edge[3] == F(0.5)
    assert np.isnan(ref.sigmoid_defined(np.array([np.nan], F))[0]) and np.isnan(ref.exp_defined(np.array([np.nan], F))[0])
    # where the unclamped f32 formula 1 / (1 + fl(exp(-v))) saturates, the defined one does, and nowhere else
    v = np.linspace(-95.0, 25.0, 24001).astype(F)
    with np.errstate(over="ignore"):
        formula = (F(1.0) / (F(1.0) + np.exp(-v.astype(np.float64)).astype(F))).astype(F)
    got = ref.sigmoid_defined(v)
    near = (np.abs(v - F(-88.7228)) < 0.01) | (np.abs(v - F(16.6355)) < 0.01)         # 2 ulp of exp may move the two thresholds
    assert np.array_equal((got == 1.0)[~near], (formula == 1.0)[~near]) and np.array_equal((got == 0.0)[~near], (formula == 0.0)[~near])


def test_one_step_worked_out_by_hand():
    """A 2 -> 1 model, x = [0, 1], alpha = 0.5.  |min - max| = 1 is not below 1e-8, so y = x.
    Case A: W_enc = [[0], [0]], b_enc = [0], W_dec = [[2, -2]], b_dec = [0, 0].
      latent = 0; la = 1 / (1 + exp(0)) = 0.5 (the defined exp gives exactly 1 at 0); output = 0 * [2, -2] + 0 = [0, 0]; act = [.5, .5].
      delta_out = ((y - act) * -1) * (act (1 - act)) = ((-.5, .5) * -1) * .25 = (.125, -.125).
      delta_dec = (.125 * 2 + -.125 * -2) * (la (1 - la)) = .5 * .25 = .125.
      W_dec -= (latent^T delta_out) alpha = 0: unchanged, because the decoder's gradient uses the PRE-activation latent, here 0.
      W_enc -= (x^T delta_dec) alpha: [[0], [-.0625]]; b_enc -= .125 * .5: [-.0625]; b_dec -= (.125, -.125) * .5: [-.0625, .0625].
      error = 0.5 sqrt(.25 + .25) = 0.5 sqrt(.5).
    Case B: b_enc = [1], b_dec = [-2, 2]: latent = 1, output = 1 * [2, -2] + [-2, 2] = [0, 0] again, so delta_out is as in A, and
      W_dec -= (1 * (.125, -.125)) * .5 = [[1.9375, -1.9375]]; b_dec = [-2.0625, 2.0625]."""
    a = ref.Model([[0.0], [0.0]], [[2.0, -2.0]], [0.0], [0.0, 0.0])
    err = a.step(np.array([0.0, 1.0], F), 0.5)
    assert a.we.ravel().tolist() == [0.0, -0.0625] and a.be.tolist() == [-0.0625]
    assert a.wd.ravel().tolist() == [2.0, -2.0] and a.bd.tolist() == [-0.0625, 0.0625]
    assert err == F(0.5) * np.sqrt(F(0.5)) and a.total_err == err and (a.steps, a.first_nonfinite) == (1, None)
    b = ref.Model([[0.0], [0.0]], [[2.0, -2.0]], [1.0], [-2.0, 2.0])
    b.step(np.array([0.0, 1.0], F), 0.5)
    assert b.wd.ravel().tolist() == [1.9375, -1.9375] and b.bd.tolist() == [-2.0625, 2.0625]


def test_norm_quirk_constant_frames_poison_the_model():
    """numerics.rs:196 rescales only when |min - max| < 1e-8, i.e. divides by (nearly) zero: a constant finite frame is 0 / 0."""
    assert np.array_equal(ref.norm(np.array([1.0, 2.0, 4.0], F)), np.array([1.0, 2.0, 4.0], F))
    assert np.isnan(ref.norm(np.array([3.0, 3.0, 3.0], F))).all()
    got = ref.norm(np.array([np.inf, 3.0, 3.0], F))                    # min and max skip the infinity: 3 and 3 -> rescaled
    assert np.isinf(got[0]) and np.isnan(got[1:]).all()
    assert np.array_equal(ref.norm(np.array([np.inf, 1.0, 2.0], F)), np.array([np.inf, 1.0, 2.0], F))      # 1 and 2: untouched
    assert np.array_equal(ref.norm(np.array([np.inf, -np.inf], F)), np.array([np.inf, -np.inf], F))         # no finite value: |inf - -inf|
    rng = np.random.default_rng(5)
    model = ref.seeded(rng, 3, 2)
    frames = rng.standard_normal((8, 3)).astype(F)
    frames[5] = 0.25
    model.run(frames, range(8), 0.1)
    assert model.first_nonfinite == 5 and model.steps == 8
    assert all(np.isnan(a).all() for a in (model.we, model.wd, model.be, model.bd)) and np.isnan(model.total_err)
    one = ref.seeded(rng, 1, 1)                                        # D = 1: every finite frame is constant
    one.step(np.array([0.7], F), 0.1)
    assert one.first_nonfinite == 0 and np.isnan(one.we).all()


def test_f32_count_sticks_at_two_to_the_24():
    from audio_pattern_discovery_amd.neural import epoch_count
    assert F(1 << 24) + F(1.0) == F(1 << 24)                           # why the reference's `total += 1.0` stops growing
    assert ref.f32_count(1000) == epoch_count(1000) == F(1000.0)
    assert epoch_count(0) == F(0.0) and epoch_count((1 << 24) - 1) == F(16777215.0)
    assert epoch_count(1 << 24) == epoch_count((1 << 24) + 5) == epoch_count(16_800_000 * 25) == F(16777216.0)


def test_step_decay_at_the_shipped_configuration(apd):
    from audio_pattern_discovery_amd.discovery import Discovery
    from audio_pattern_discovery_amd.neural import AutoEncoder
    cfg = Discovery()                                                  # learning_rate 0.1, drop 0.5, epoch_drop 5.0
    want = {0: F(0.1), 3: F(0.1), 4: F(0.1) * F(0.5), 9: F(0.1) * F(0.25)}
    for epoch, lr in want.items():
        assert F(AutoEncoder.step_decay(epoch, cfg)) == lr == ref.step_decay(0.1, 0.5, 5.0, epoch)
    assert F(apd.lib().apd_step_decay(0.1, 0.5, 5.0, 24.0)) == F(0.1) * F(0.03125)


def test_train_order_is_the_checkers_and_a_shuffle_per_signal(apd):
    from audio_pattern_discovery_amd.neural import train_order
    offsets = np.array([0, 40, 40, 41, 300, 300, 1000], np.uint64)     # empty signals, a signal of one frame
    seen = []
    for seed, epoch in ((0, 0), (0, 1), (7, 0), (2 ** 63 + 11, 2 ** 40)):
        got = train_order(seed, epoch, offsets)
        assert got.dtype == np.uint32 and np.array_equal(got, ref.train_order(seed, epoch, offsets))
        for s in range(len(offsets) - 1):
            a, b = int(offsets[s]), int(offsets[s + 1])
            assert np.array_equal(np.sort(got[a:b]), np.arange(a, b))          # a permutation of the signal's own frames
        assert got.tobytes() == train_order(seed, epoch, offsets).tobytes()
        seen.append(got.tobytes())
    assert len(set(seen)) == 4                                         # epochs and seeds differ
    assert not np.array_equal(train_order(0, 0, offsets)[41:300], np.arange(41, 300))
    shifted = train_order(3, 2, np.array([100, 130], np.uint64))       # frame numbers are absolute, the array starts at 0
    assert np.array_equal(np.sort(shifted), np.arange(100, 130))
    assert train_order(1, 1, np.zeros(0, np.uint64)).size == 0 and train_order(1, 1, np.array([5, 5, 5], np.uint64)).size == 0
    L = apd.lib()
    assert L.apd_train_order(1, 1, None, 0, None) == apd.APD_OK
    bad = np.array([0, 9, 4], np.uint64)
    assert L.apd_train_order(1, 1, bad.ctypes.data_as(C.POINTER(C.c_uint64)), 2, np.zeros(16, np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))) == apd.APD_ERR_INVALID_ARG
    assert L.apd_train_order(1, 1, None, 2, None) == apd.APD_ERR_INVALID_ARG
    huge = np.array([0, 1 << 32], np.uint64)
    assert L.apd_train_order(1, 1, huge.ctypes.data_as(C.POINTER(C.c_uint64)), 1, None) == apd.APD_ERR_INVALID_ARG


def test_cpp_restatement_under_the_sanitizers_gives_the_checkers_bits(tmp_path):
    """tools/train_cpu.cpp with csrc/train_host.hip, plain C++ under AddressSanitizer + UBSan (a CPU build, its own process): 300 steps
    at 13 -> 8 with a constant frame late in the order, and at 5 -> 33; apd_train_order and apd_step_decay through the same program."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "train_cpu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-x", "c++", os.path.join(ROOT, "tools", "train_cpu.cpp"), "-o", exe])
    for d, l, poison in ((13, 8, 290), (5, 33, None)):
        rng = np.random.default_rng(d * 100 + l)
        model = ref.seeded(rng, d, l)
        frames = (rng.standard_normal((120, d)) * 2.0).astype(F)
        order = rng.integers(0, 119, 300).astype(np.uint32)           # repeats; frame 119 is reached only as the poison
        if poison is not None:
            frames[119] = -1.5
            order[poison] = 119
        case = tmp_path / ("case_%d_%d.bin" % (d, l))
        with open(case, "wb") as fp:
            fp.write(np.array([d, l, 120, 300], np.uint32).tobytes() + F(0.1).tobytes())
            for a in (model.we, model.wd, model.be, model.bd, frames, order):
                fp.write(np.ascontiguousarray(a).tobytes())
        out = subprocess.run([exe, "run", str(case)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-3000:]
        words = out.stdout.split()
        model.run(frames, order, 0.1)
        n = 2 * d * l + d + l
        assert np.array_equal(ref.canonical_bits(np.array([int(w, 16) for w in words[:n]], np.uint32).view(F)), model.bits())
        assert ref.canonical_bits(np.array([int(words[n], 16)], np.uint32).view(F))[0] == ref.canonical_bits([model.total_err])[0]
        assert int(words[n + 1]) == 300 and int(words[n + 2]) == (-1 if poison is None else poison) and model.first_nonfinite == poison
    out = subprocess.run([exe, "order", "7", "3", "0", "40", "40", "41", "300"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-3000:]
    assert [int(w) for w in out.stdout.split()] == ref.train_order(7, 3, [0, 40, 40, 41, 300]).tolist()
    assert subprocess.run([exe, "order", "7", "3"], capture_output=True, text=True, timeout=60).stdout == ""
    out = subprocess.run([exe, "decay", "0.1", "0.5", "5.0", "9"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and int(out.stdout, 16) == int(np.array([F(0.1) * F(0.25)], F).view(np.uint32)[0])
