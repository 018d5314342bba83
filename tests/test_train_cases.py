"""CPU tests of the trainer's case table (tests/_train_cases.py; DESIGN.md section 4.18, "Tests"): on the checker alone, that every
case reaches what it is there for -- the sigmoid arguments are observed in the compared bits, an intermediate is subnormal and a
flush-to-zero checker ends elsewhere, a dot product turns NaN through +inf - inf, Mat::norm takes the stated branch, rates and
starting weights end finite or not at the stated step, a weight is inf before any is NaN -- so that a device which equals the
checker on these cases (tests/test_gpu_train_edges.py) has been through them.  No GPU, no library."""
import contextlib
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import _train_cases as cases
import _train_reference as ref

F = np.float32
TINY = np.finfo(F).tiny
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_case_builds_and_stays_in_its_frames():
    """Every order index is a frame of the case, every model of a case has one shape, and building a case twice gives the same bytes."""
    for name in cases.names():
        if name.startswith(("512 models", "1500 models")):
            continue                                                       # built by test_many_models_* below
        case = cases.get(name)
        shapes = {(m.we.shape, m.wd.shape, m.be.shape, m.bd.shape) for m in case.models}
        assert len(shapes) == 1, name
        d = case.models[0].bd.size
        assert case.frames.ndim == 2 and case.frames.shape[1] == d, name
        for order, alpha in case.runs:
            assert order.ndim in (1, 2) and (order.ndim == 1 or order.shape[0] == len(case.models)), name
            assert alpha.shape == (len(case.models),), name
            assert order.size == 0 or order.max() < len(case.frames), name
        builder, args = cases.BUILDERS[name]
        again = builder(*args)
        assert again.frames.tobytes() == case.frames.tobytes() and all(np.array_equal(a.bits(), b.bits()) for a, b in zip(again.models, case.models)), name


# ---- 1. the sigmoid --------------------------------------------------------------------------------------------------------------
def sigmoid_arguments_seen_by_the_checker(case):
    """The arguments the checker's sigmoid receives at the case's call site, [model][64]."""
    call, out = {"la": 0, "act": 1}[case.info["site"]], []
    for model in case.models:
        got = []

        def sigmoid(v, got=got):
            got.append(np.array(v, F))
            return ref.sigmoid_defined(v)

        ref.Model(model.we, model.wd, model.be, model.bd, F, sigmoid).step(case.frames[0], 1.0)
        out.append(got[call])
    return np.stack(out)


@pytest.mark.parametrize("site", ["act", "la"])
def test_the_probes_hand_their_arguments_to_the_sigmoid_unchanged(site):
    """Lane i of model m evaluates sigmoid(args[m][i]) at the probed call site, bit for bit -- but for -0, which no step can hand to
    the sigmoid: its argument is a sum that starts from +0.0, and +0 + -0 = +0 (the -0 bias is still part of the compared state)."""
    for part in ("edges", "sweep"):
        case = cases.get("sigmoid %s %s" % (site, part))
        want = case.info["args"].view(np.uint32).copy()
        assert ((want == 0x80000000).sum() > 0) == (part == "edges")
        want[want == 0x80000000] = 0
        assert np.array_equal(sigmoid_arguments_seen_by_the_checker(case).view(np.uint32), want)
        assert case.runs[0][0].tolist() == [0] and (case.runs[0][1] == 1.0).all() and len(case.frames) == 1


def test_the_edge_list_covers_what_train_exp_does():
    """The list holds the named edges, and its arguments reach every stage of train_exp: both clamps, kf ties that round up and ties
    that round down, subnormal and infinite e, subnormal quotients, results exactly 0, 0.5 and 1."""
    edges = cases.sigmoid_edges()
    present = set(edges.view(np.uint32).tolist())
    for v in (0.0, -0.0, 1e-45, -1e-45, TINY, -TINY, 100.0, -100.0, 104.0, -104.0, cases.FLT_MAX, -cases.FLT_MAX):
        for u in cases.ulps(v, 1):
            assert int(F(u).view(np.uint32)) in present, u
    t = -edges
    assert (t > 100).any() and (t < -104).any()
    with np.errstate(all="ignore"):
        tc = np.clip(t, F(-104.0), F(100.0))
        z = tc * F(1.44269504)
        kf = (z + F(12582912.0)) - F(12582912.0)
        e, s = ref.exp_defined(t), ref.sigmoid_defined(edges)
    tie = np.abs(z - np.floor(z) - F(0.5)) == 0
    assert (tie & (kf > z)).sum() >= 20 and (tie & (kf < z)).sum() >= 20          # exact ties, rounded to the even neighbour either way
    assert set(range(-150, 145)) <= set(kf.astype(int).tolist())
    assert ((e > 0) & (e < TINY)).sum() >= 100 and np.isinf(e).sum() >= 10 and (e[t < -104] == 0).all() and (e[t > -103] > 0).all()
    assert ((s > 0) & (s < TINY)).sum() >= 100
    assert (s == 0).any() and (s == 1).any() and (s == F(0.5)).any()
    assert np.signbit(edges[s == F(0.5)]).any() and not np.signbit(edges[s == F(0.5)]).all()
    assert np.array_equal(np.sort(edges[(edges > -88.81) & (edges < -87.29)])[[0, -1]].round(1), F([-88.8, -87.3]))


def test_the_sweep_covers_every_binary_exponent_and_both_bands():
    sweep = cases.sigmoid_sweep(np.random.default_rng(181))
    fields = (sweep.view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF)
    for sign in (False, True):
        assert set(range(0, 135)) <= set(fields[np.signbit(sweep) == sign].tolist())
    assert ((sweep >= -105) & (sweep <= -86)).sum() >= 1000 and ((sweep >= -30) & (sweep <= 30) & (np.abs(sweep) > 1e-3)).sum() >= 1000
    assert 3000 <= sweep.size + cases.sigmoid_edges().size <= 6000


def observed_share(name):
    case = cases.get(name)
    seen = cases.observed(case.info["site"], case.models, case.frames[0])
    used = case.info["used"]
    return case, seen, used


def test_act_site_every_edge_argument_is_observed():
    """An argument is observed if replacing the checker's sigmoid value there by its upper neighbour changes a compared bit, and so
    does replacing it by its lower neighbour.  Every argument of the edge list is, in the lane it was given."""
    case, seen, used = observed_share("sigmoid act edges")
    edges = cases.sigmoid_edges()
    assert used.sum() == edges.size
    assert np.array_equal(np.sort(case.info["args"][used].view(np.uint32)), np.sort(edges.view(np.uint32)))
    assert seen[used].all(), case.info["args"][used & ~seen]


def test_act_site_sweep_is_observed():
    case, seen, used = observed_share("sigmoid act sweep")
    share = seen[used].mean()
    print("act site: %d of %d sweep arguments observed (%.1f %%)" % (seen[used].sum(), used.sum(), 100 * share))
    assert share >= 0.95


def test_la_site_sweep_is_observed():
    """la enters the step through la (1 - la) alone, which is 0.25 for every neighbour of 0.5: arguments below ~ 1e-7 in size cannot
    be observed at this site, whatever the probe."""
    case, seen, used = observed_share("sigmoid la sweep")
    share = seen[used].mean()
    print("la site: %d of %d sweep arguments observed (%.1f %%)" % (seen[used].sum(), used.sum(), 100 * share))
    assert share >= 0.70
    case, seen, used = observed_share("sigmoid la edges")
    print("la site: %d of %d edge arguments observed" % (seen[used].sum(), used.sum()))


@pytest.mark.parametrize("site", ["act", "la"])
def test_non_finite_sigmoid_arguments_poison_at_step_0(site):
    case = cases.get("sigmoid %s non-finite" % site)
    args = sigmoid_arguments_seen_by_the_checker(case)
    assert np.isposinf(args[0, 0]) and np.isneginf(args[1, 63]) and np.isnan(args[2, 31])
    assert [m.first_nonfinite for m in case.trained()[0]] == [0, 0, 0]


# ---- 2. arithmetic that leaves the normal range -----------------------------------------------------------------------------------
@contextlib.contextmanager
def mul_row_as(flush, seen):
    """Replaces the checker's mul_row: `seen` collects whether a product or a partial sum was subnormal and not zero; with `flush`
    such a result becomes a zero of its sign after each operation (what a flush-to-zero device would compute)."""
    def after(v):
        sub = (np.abs(v) < TINY) & (v != 0)
        if sub.any():
            seen.append(True)
        return np.where(sub, np.copysign(F(0.0), v), v).astype(F) if flush else v

    def mul_row(x, w):
        acc = np.zeros(w.shape[1], w.dtype)
        for k in range(w.shape[0]):
            acc = after(acc + after(x[k] * w[k]))
        return acc

    saved, ref.mul_row = ref.mul_row, mul_row
    try:
        yield
    finally:
        ref.mul_row = saved


def run_fresh(case):
    models = [m.copy() for m in case.models]
    for order, alpha in case.runs:
        for m, model in enumerate(models):
            model.run(case.frames, order[m] if order.ndim == 2 else order, alpha[m])
    return models


@pytest.mark.parametrize("shape", ["5->3", "13->8"])
def test_subnormal_products_reach_the_final_bits(shape):
    case = cases.get("subnormal products " + shape)
    want = case.trained()[-1][0]
    assert want.first_nonfinite is None and np.isfinite(case.frames).all()
    seen = []
    with mul_row_as(False, seen):
        same = run_fresh(case)[0]
    assert seen and np.array_equal(same.bits(), want.bits()) and same.total_err.view(np.uint32) == want.total_err.view(np.uint32)
    with mul_row_as(True, []):
        flushed = run_fresh(case)[0]
    assert not np.array_equal(flushed.bits(), want.bits())
    sub = lambda a: int(((np.abs(a) < TINY) & (a != 0)).sum())
    assert sub(want.we) + sub(want.wd) > 0                                 # and subnormal weights are part of the compared state


def test_dot_overflow_is_nan_because_k_ascends():
    case = cases.get("dot overflow")
    x, w, step = case.info["frame"], case.info["column"], case.info["step"]
    with np.errstate(all="ignore"):
        up = down = F(0.0)
        partial = []
        for k in range(5):
            up = up + x[k] * w[k]
            partial.append(up)
        for k in reversed(range(5)):
            down = down + x[k] * w[k]
        third = x[2] * w[2]
    assert np.isfinite(x).all() and np.isfinite(w).all()
    assert np.isfinite(partial[0]) and np.isposinf(partial[1]) and np.isneginf(third) and np.isnan(partial[2]) and np.isnan(up)
    assert np.isneginf(down)
    trained = case.trained()[0][0]
    assert trained.first_nonfinite == step and case.runs[0][0][step] == 9
    before = case.models[0].copy().run(case.frames, case.runs[0][0][:step], 0.0)
    assert np.array_equal(before.we[:, 0], w) and before.finite()


@pytest.mark.parametrize("shape", ["5->3", "13->8"])
def test_huge_frames_tiny_weights_and_signed_zeros(shape):
    huge = cases.get("huge frames " + shape)
    assert np.abs(huge.frames).max() > 1e30 and np.isfinite(huge.frames).all()
    slow, fast = huge.trained()[0]
    assert slow.first_nonfinite is None and fast.first_nonfinite is not None   # one stays finite to the end, one overflows on the way
    tiny = cases.get("tiny weights " + shape)
    for a in (tiny.models[0].we, tiny.models[0].wd, np.concatenate([tiny.models[0].be, tiny.models[0].bd])):
        assert (np.abs(a) < TINY).all() and (a == 0).any() and (a != 0).any() and np.signbit(a[a == 0]).any() and not np.signbit(a[a == 0]).all()
    assert tiny.trained()[0][0].first_nonfinite is None
    zeros = cases.get("signed zeros " + shape)
    assert (zeros.runs[0][1] == 0).all() and np.signbit(zeros.frames[zeros.frames == 0]).any()
    for start, end in zip(zeros.models, zeros.trained()[0]):
        # w - g * 0 with g finite: every non-zero weight keeps its bits and a zero stays a zero.  -0 - (+0) = -0 keeps a -0; where a
        # gradient was negative, g * 0 = -0 and -0 - (-0) = +0 does not, and the device must lose the sign in the same places.
        assert end.first_nonfinite is None
        a, b = start.bits(), end.bits()
        nonzero = (a & 0x7FFFFFFF) != 0
        assert np.array_equal(a[nonzero], b[nonzero]) and ((b[~nonzero] & 0x7FFFFFFF) == 0).all()
    print("signed zeros %s: -0 weights kept %d of %d (a third -0), %d of %d (all -0)" % ((shape,) + sum(
        [(int((e.bits() == 0x80000000).sum()), int((s.bits() == 0x80000000).sum())) for s, e in zip(zeros.models, zeros.trained()[0])], ())))


# ---- 3. Mat::norm ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [5, 64])
def test_norm_takes_the_stated_branch(d):
    for name, (x, rescales, _) in cases.norm_frames(d).items():
        y = ref.norm(x)
        took = not np.array_equal(ref.canonical_bits(y), ref.canonical_bits(x))
        assert took == rescales, name
    frames = cases.norm_frames(d)
    y = ref.norm(frames["spread below 1e-8"][0])[:5]
    assert np.array_equal(y, F([0, F(3e-9) / F(9e-9), F(7e-9) / F(9e-9), 1, F(1e-9) / F(9e-9)])) and np.allclose(y, [0, 1 / 3, 7 / 9, 1, 1 / 9])
    assert set(ref.norm(frames["one ulp apart at 0.05"][0]).tolist()) == {0.0, 1.0}
    y = ref.norm(frames["subnormal spread"][0])[:5]
    x = frames["subnormal spread"][0][:5]
    assert 0 < x.max() < TINY and np.array_equal(y, x / x.max()) and set(y.tolist()) == {0.0, 0.5, 1.0}   # 1e-45, 2e-45 and 3e-45 are 1, 1 and 2 units of 2^-149
    y = ref.norm(frames["inf and a spread below 1e-8"][0])
    assert np.isposinf(y[0]) and np.isfinite(y[1:]).all() and y[1:].min() == 0 and y[1:].max() == 1
    s = frames["spread just under 1e-8"][0]
    assert s.max() - s.min() == np.nextafter(F(1e-8), F(0)) and frames["spread exactly 1e-8"][0].max() == F(1e-8)
    for name in ("repeated ends, min first", "repeated ends, max first", "repeated ends, wide"):
        x = frames[name][0]
        assert (x == x.min()).sum() >= 2 and (x == x.max()).sum() >= 2
        assert {x[0], x[1], x[-1], x[-2]} == {x.min(), x.max()}


@pytest.mark.parametrize("name", ["norm 5->3", "norm 64->7"])
def test_norm_frames_leave_the_model_finite_or_not_as_stated(name):
    case = cases.get(name)
    d = case.frames.shape[1]
    special = cases.norm_frames(d)
    orders = case.runs[0][0]
    trained = case.trained()[0]
    n_plain = len(case.frames) - len(special)
    assert set(cases.NORM_PLACES) == {0, 7, 11} and orders.shape[1] == 20
    for m, at in enumerate(case.info["at"]):
        hits = np.flatnonzero(orders[m] >= n_plain)
        if at is None:
            assert hits.size == 0 and trained[m].first_nonfinite is None
            alone = case.models[m].copy().run(case.frames[:n_plain], orders[m], case.runs[0][1][m])
            assert np.array_equal(alone.bits(), trained[m].bits())
            continue
        frame_name, step = at
        assert hits.tolist() == [step] and np.array_equal(ref.canonical_bits(case.frames[orders[m, step]]), ref.canonical_bits(special[frame_name][0]))
        finite = special[frame_name][2]
        if finite is not None:
            assert trained[m].first_nonfinite == (None if finite else step), case.labels[m]


# ---- 4. rates, starting weights, the first non-finite step ------------------------------------------------------------------------
def test_rates_end_finite_or_not_as_stated():
    case = cases.get("rates")
    alpha = case.runs[0][1]
    assert alpha[0] == 0 and alpha[1] < 0 and 0 < alpha[2] < TINY and alpha[3] == F(1e30) and np.isposinf(alpha[4]) and np.isnan(alpha[5])
    assert [m.first_nonfinite for m in case.trained()[0]] == cases.RATES_FIRST_NONFINITE == [None, None, None, 1, 0, 0]


@pytest.mark.parametrize("shape", ["64->64", "33->5", "5->33"])
def test_one_non_finite_starting_weight_is_found_at_step_0(shape):
    """Twelve places, one model each: exactly one starting value is not finite, the checker reports step 0 -- and in some of them the
    value never spreads, so that only the tracking of that array and lane can report it."""
    contained = 0
    for steps in (1, 8, 9):
        case = cases.get("non-finite start %s, %d steps" % (shape, steps))
        assert len(case.models) == 12 and case.runs[0][0].size == steps
        for model, trained in zip(case.models, case.trained()[0]):
            w = np.concatenate([a.ravel() for a in (model.we, model.wd, model.be, model.bd)])
            assert (~np.isfinite(w)).sum() == 1
            assert trained.first_nonfinite == 0 and trained.steps == steps
            after = np.concatenate([a.ravel() for a in (trained.we, trained.wd, trained.be, trained.bd)])
            contained += int((~np.isfinite(after)).sum() == 1)
    print("%s: in %d of 36 runs the non-finite value stays alone" % (shape, contained))
    assert contained >= 3


def test_a_weight_is_inf_before_any_is_nan():
    history = cases.diverge_history()
    s = cases.diverge_inf_step()
    assert history[s] == (True, False) and not any(inf or nan for inf, nan in history[:s])
    assert any(nan for _, nan in history[s + 1:]) and 0 < s < len(history) - 1
    whole, last, first = (cases.get("diverge " + k) for k in ("whole", "last", "first"))
    assert len(last.runs[0][0]) == s + 1 and len(first.runs[0][0]) == s
    end = whole.trained()[-1][0]
    assert end.first_nonfinite == s
    for split in (last, first):
        got = split.trained()[-1][0]
        assert got.first_nonfinite == s and np.array_equal(got.bits(), end.bits()) and got.steps == end.steps
    assert last.trained()[0][0].first_nonfinite == s and first.trained()[0][0].first_nonfinite is None


# ---- 5. step counts ----------------------------------------------------------------------------------------------------------------
def test_step_count_cases_are_the_stated_ones():
    assert cases.RUN_LENGTHS == (7, 8, 9, 15, 16, 17, 24, 25, 64) and cases.CONTINUATIONS == ((8, 8), (8, 1), (7, 9), (16, 0, 8))
    for d, l in ((3, 2), (13, 8)):
        for lengths in [(n,) for n in cases.RUN_LENGTHS] + list(cases.CONTINUATIONS):
            for per_model in (False, True):
                case = cases.get("%s steps %d->%d %s" % (" + ".join(map(str, lengths)), d, l, "per model" if per_model else "shared"))
                assert [o.shape[-1] for o, _ in case.runs] == list(lengths)
                assert case.models[0].we.shape == (d, l) and len(case.models) == (3 if per_model else 2)
                last = len(case.frames) - 1
                for order, _ in case.runs:
                    assert order.ndim == (2 if per_model else 1)
                    for row in np.atleast_2d(order):
                        assert row.size == 0 or (row[-1] == last and (0 in row or row.size < 3))
                if per_model:
                    assert all((m * n) % 8 for n in lengths for m in (1, 2) if n % 8)
                assert all(m.first_nonfinite is None for m in case.trained()[-1])


# ---- 6. many models ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("512 models 64->64", 512), ("1500 models 3->2", 1500)])
def test_many_models_have_their_own_starts_rates_and_orders(name, n):
    case = cases.get(name)
    order, alpha = case.runs[0]
    assert len(case.models) == n and order.shape == (n, 9) and case.info["alone"] == (0, n // 2, n - 1)
    assert len({m.bits().tobytes() for m in case.models}) == n and len(set(alpha.tolist())) > n // 2 and len({o.tobytes() for o in order}) > n // 2
    assert all(m.first_nonfinite is None and m.steps == 9 for m in case.trained()[0])


# ---- a second witness ----------------------------------------------------------------------------------------------------------------
def test_the_cpp_restatement_ends_every_case_in_the_checkers_bits(tmp_path):
    """tools/train_cpu.cpp (csrc/train_math.h compiled for the host, -ffp-contract=off) on every model of every case but the two large
    launches, the runs of a case joined into one order: the weights, total_err and the first non-finite step are the checker's.  The
    checker restates train_math.h; this is the text itself, at the arguments the device is held to."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe, path = str(tmp_path / "train_cpu"), str(tmp_path / "case.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-x", "c++", os.path.join(ROOT, "tools", "train_cpu.cpp"), "-o", exe])
    checked = 0
    for name in cases.names():
        if " models " in name:
            continue
        case = cases.get(name)
        for m, (model, want) in enumerate(zip(case.models, case.trained()[-1])):
            order = np.concatenate([o[m] if o.ndim == 2 else o for o, _ in case.runs]).astype(np.uint32)
            alpha = case.runs[0][1][m]
            assert all(a[m].tobytes() == alpha.tobytes() for _, a in case.runs)
            with open(path, "wb") as f:
                f.write(struct.pack("<4I", model.bd.size, model.be.size, len(case.frames), order.size) + alpha.tobytes())
                for a in (model.we, model.wd, model.be, model.bd, case.frames, order):
                    f.write(np.ascontiguousarray(a).tobytes())
            out = subprocess.run([exe, "run", path], check=True, capture_output=True, text=True).stdout.split()
            words = np.array([int(w, 16) for w in out[:-2]], np.uint32).view(F)
            assert np.array_equal(ref.canonical_bits(words), np.concatenate([want.bits(), ref.canonical_bits([want.total_err])])), (name, case.labels[m])
            assert (int(out[-2]), None if int(out[-1]) < 0 else int(out[-1])) == (want.steps, want.first_nonfinite), (name, case.labels[m])
            checked += 1
    assert checked > 500
