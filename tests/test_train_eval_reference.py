"""CPU tests of apd_trainer_evaluate's definition: the checker of tests/_train_eval_reference.py against
Model.step under a rate of zero, an answer worked out by hand, constant frames (an error of their own, nothing else), the lemma the
GPU test's sigmoid probe rests on, and the single-thread C++ restatement (tools/train_eval_cpu.cpp, built with csrc/train_math.h
under AddressSanitizer + UBSan and run as a program) against the checker's bits.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _train_eval_reference as ev
import _train_reference as ref

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Share of the FINITE probe arguments at which error == 0.5 * sigmoid(u) exactly (the lemma of _train_eval_reference): computed by
# test_probe_lemma below from the checker alone.  tests/test_gpu_train_eval.py holds the same figure as its floor.
PROBE_OBSERVED_FLOOR = 0.9094


@pytest.mark.parametrize("d,l", [(3, 2), (13, 8), (64, 64)])
def test_checker_is_the_forward_half_of_model_step(d, l):
    """Finite models, no constant frame, 200 positions with repeats: the errors are Model.step's return values at alpha = 0, the total
    its total_err, and the copy that took the steps still has the weights it started with."""
    rng = np.random.default_rng(9000 + 100 * d + l)
    model = ref.seeded(rng, d, l)
    frames = (rng.standard_normal((70, d)) * 2.0).astype(F)
    order = rng.integers(0, 70, 200).astype(np.uint32)
    errors, total, first = ev.evaluate(model, frames, order)
    stepped = model.copy()
    want = np.array([stepped.step(frames[int(i)], 0.0) for i in order], F)
    assert np.array_equal(ref.canonical_bits(errors), ref.canonical_bits(want))
    assert ref.canonical_bits([total])[0] == ref.canonical_bits([stepped.total_err])[0] and first is None and np.isfinite(total)
    ran = model.copy().run(frames, order, 0.0)
    assert ref.canonical_bits([ran.total_err])[0] == ref.canonical_bits([total])[0]
    for a, b in ((ran.we, model.we), (ran.wd, model.wd), (ran.be, model.be), (ran.bd, model.bd)):
        assert np.array_equal(a, b)                      # in value: w - 0 * g may turn a -0 into +0


def test_one_evaluation_worked_out_by_hand():
    """A 2 -> 1 model, x = [0, 1]: |min - max| = 1 is not below 1e-8, so y = x.
    W_enc = [[3], [2]], b_enc = [-2]: latent = (0 + 0 * 3) + 1 * 2 + -2 = 0.
    W_dec = [[5, -7]], b_dec = [0, 0]: output = 0 * [5, -7] + [0, 0] = [0, -0 + 0] = [0, 0]; act = sigmoid(0) = [.5, .5] (the defined
    exp gives exactly 1 at 0).  diff = act - y = [.5, -.5]; squares .25 + .25 = .5; error = 0.5 * sqrt(.5).
    With b_enc = [-1]: latent = 1, output = [5, -7]: the error is 0.5 * sqrt(s(5)^2 + (s(-7) - 1)^2), from the defined sigmoid.
    Two positions of the first model: total = e + e, first_nonfinite none."""
    x = np.array([[0.0, 1.0]], F)
    a = ref.Model([[3.0], [2.0]], [[5.0, -7.0]], [-2.0], [0.0, 0.0])
    e = F(0.5) * np.sqrt(F(0.5))
    assert ev.error_of(a, x[0]) == e
    errors, total, first = ev.evaluate(a, x, [0, 0])
    assert errors.tolist() == [e, e] and total == F(e + e) and first is None
    b = ref.Model([[3.0], [2.0]], [[5.0, -7.0]], [-1.0], [0.0, 0.0])
    s = ref.sigmoid_defined(np.array([5.0, -7.0], F))
    d0, d1 = F(s[0] - F(0.0)), F(s[1] - F(1.0))
    assert ev.error_of(b, x[0]) == F(F(0.5) * np.sqrt(F(F(F(0.0) + F(d0 * d0)) + F(d1 * d1))))
    assert ev.evaluate(a, np.zeros((0, 2), F))[1:] == (F(0.0), None)


@pytest.mark.parametrize("d", [1, 5])
def test_constant_frames_cost_their_own_position_only(d):
    rng = np.random.default_rng(9100 + d)
    model = ref.seeded(rng, d, 3)
    frames = (rng.standard_normal((9, d)) * 2.0).astype(F)
    frames[4] = 0.25
    before = [a.copy() for a in (model.we, model.wd, model.be, model.bd)]
    arrays = (model.we, model.wd, model.be, model.bd)
    errors, total, first = ev.evaluate(model, frames)
    constant = np.array([np.ptp(f) == 0 for f in frames])             # at D = 1 every frame is
    assert np.array_equal(np.isnan(errors), constant) and constant[4]
    assert first == int(np.argmax(constant)) and np.isnan(total)
    assert np.isfinite(ev.evaluate(model, frames[:first])[1])          # the total is finite up to that position, NaN from it on
    assert np.isnan(ev.evaluate(model, frames[:first + 1])[1])
    for a, b, c in zip(arrays, before, (model.we, model.wd, model.be, model.bd)):
        assert a is c and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    poisoned = model.copy().run(frames, range(9), 0.0)                 # the route the parent had: alpha = 0 poisons the model
    assert not poisoned.finite() and model.finite()


def test_probe_lemma():
    """error == 0.5 * sigmoid_defined(u) wherever sigmoid(u)^2 is a normal f32; the share of the probe's finite arguments at which it
    holds is the floor the GPU test asserts."""
    args, n = ev.probe_arguments()
    flat = args.ravel()[:n]
    holds = ev.probe_lemma_holds(flat)
    s = ref.sigmoid_defined(flat)
    with np.errstate(all="ignore"):
        normal_square = (s * s) >= np.finfo(F).tiny
    assert holds[normal_square].all()                                  # the lemma, at every argument it speaks of
    assert holds[np.isnan(flat)].all() and holds[flat == np.inf].all()
    finite = np.isfinite(flat)
    share = holds[finite].mean()
    print("probe: %d arguments, %d finite, lemma holds at %d of them (%.4f); %d where it does not are compared anyway"
          % (n, finite.sum(), holds[finite].sum(), share, (~holds[finite]).sum()))
    assert share >= PROBE_OBSERVED_FLOOR
    # and the probe does what its comment says: y = x, act_1 = 1 exactly
    assert ref.sigmoid_defined(np.array([40.0], F))[0] == F(1.0) and np.array_equal(ref.norm(ev.PROBE_FRAME[0]), ev.PROBE_FRAME[0])


def special_frames(d):
    """Frames that rescale, a NaN frame and an infinite one, for any d >= 3."""
    tile = lambda v: np.resize(np.asarray(v, F), d)
    return [tile([0, 3e-9, 7e-9, 9e-9, 1e-9]), tile([np.nan, 1.0, 2.0]), tile([np.inf, 0.5, -0.5]), tile([0.25])]


@pytest.mark.parametrize("d,l", [(1, 1), (3, 2), (13, 8), (5, 33), (64, 64)])
def test_batched_checker_has_the_scalar_checkers_bits(d, l):
    """errors_batch / evaluate_many (what the GPU tests use on many positions) against error_of / evaluate position by position:
    ordinary, huge and tiny frames, every rescaling case of the trainer's Mat::norm group, NaN, infinite and constant frames."""
    import _train_cases as cases
    rng = np.random.default_rng(9300 + 100 * d + l)
    models = [ref.seeded(rng, d, l) for _ in range(2)]
    parts = [(rng.standard_normal((30, d)) * 2.0).astype(F), (rng.standard_normal((5, d)) * 1e30).astype(F), (rng.standard_normal((5, d)) * 1e-30).astype(F),
             np.full((1, d), 0.25, F), np.full((1, d), np.nan, F), np.full((1, d), np.inf, F), np.full((1, d), -np.inf, F)]
    if d >= 5:
        parts += [np.stack([v[0] for v in cases.norm_frames(d).values()])]
    frames = np.concatenate(parts)
    order = rng.integers(0, len(frames), (2, 90)).astype(np.uint32)
    got = ev.evaluate_many(models, frames, order)
    for m, model in enumerate(models):
        errors, total, first = ev.evaluate(model, frames, order[m])
        assert np.array_equal(ref.canonical_bits(got[0][m]), ref.canonical_bits(errors))
        assert ref.canonical_bits(got[1][m:m + 1])[0] == ref.canonical_bits([total])[0] and got[2][m] == first
    whole = ev.evaluate_many(models, frames)
    assert np.array_equal(ref.canonical_bits(whole[0][1]), ref.canonical_bits(ev.evaluate(models[1], frames)[0]))


def test_cpp_restatement_under_the_sanitizers_gives_the_checkers_bits(tmp_path):
    """tools/train_eval_cpu.cpp, plain C++ under AddressSanitizer + UBSan (a CPU build, its own process): three shapes x 130 positions,
    two models each with their own order rows, a rescaling, a NaN, an infinite and a constant frame among the positions."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "train_eval_cpu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "train_eval_cpu.cpp"), "-o", exe])
    for d, l in ((3, 2), (13, 8), (64, 64)):
        rng = np.random.default_rng(9200 + d)
        models = [ref.seeded(rng, d, l) for _ in range(2)]
        frames = np.concatenate([(rng.standard_normal((40, d)) * 2.0).astype(F), np.stack(special_frames(d))])
        order = rng.integers(0, 40, (2, 130)).astype(np.uint32)
        order[0, [5, 64, 100, 129]] = [41, 40, 42, 43]
        order[1, 77] = 40                                              # finite error: the frame rescales to a spread of [0, 1]
        case = tmp_path / ("case_%d_%d.bin" % (d, l))
        with open(case, "wb") as fp:
            fp.write(np.array([d, l, 2, len(frames), 130, 1], np.uint32).tobytes())
            for m in models:
                for a in (m.we, m.wd, m.be, m.bd):
                    fp.write(np.ascontiguousarray(a).tobytes())
            fp.write(frames.tobytes() + order.tobytes())
        out = subprocess.run([exe, "run", str(case)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-3000:]
        words = out.stdout.split()
        assert len(words) == 2 * 132
        for m, model in enumerate(models):
            errors, total, first = ev.evaluate(model, frames, order[m])
            mine = words[m * 132:(m + 1) * 132]
            got = np.array([int(w, 16) for w in mine[:131]], np.uint32).view(F)
            assert np.array_equal(ref.canonical_bits(got[:130]), ref.canonical_bits(errors)), (d, l, m)
            assert ref.canonical_bits(got[130:])[0] == ref.canonical_bits([total])[0]
            assert int(mine[131]) == (-1 if first is None else first)
        assert ev.evaluate(models[0], frames, order[0])[2] == 5 and ev.evaluate(models[1], frames, order[1])[2] is None
