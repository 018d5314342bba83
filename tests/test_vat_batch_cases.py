"""CPU tests of the batched VAT case table (tests/_vat_batch_cases.py; DESIGN.md section 4.19, "Tests"): on oracle/np_reference.py
and the integer model alone, that the model with holes is the reference, and that every case reaches what it is there for -- its
NaN columns lie where its name puts them relative to the scan's 64-column wavefronts and its workgroup-wide steps, a range of the
answer spans the stretch or starts right behind it, the dense recordings emit exactly the number of ranges the device buffer is
sized for, the percentile's index sits on the last classified variance and one past it -- so that a device which equals these
answers (tests/test_gpu_vat_batch_edges.py) has been through them.  No GPU, no library."""
import numpy as np
import pytest

import _companion_cases as cc
import _vat_batch_cases as cases
from oracle import np_reference as npr

WAVE = cases.WAVE


def reference(frames, k, perc, min_len):
    try:
        return npr.interesting_ranges(frames, k, perc, min_len)
    except IndexError:
        return "panic"


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def test_without_holes_the_model_is_the_integer_model():
    for a in (cc.KAT_A, cc.random_integer_a(), cc.wrap_a(5000, seed=3)):
        for k, min_len in ((4, 3), (8, 0), (64, 10)):
            idx = cases.index_of(len(a), 0.5)
            want = cc.integer_ranges(a, k, idx, min_len)
            got = cases.hole_ranges(a, [], k, idx, min_len)
            assert got == (want[0], want[1], want[2], want[4])
            assert cases.hole_sums(a, [], k)[0].tolist() == want[3]


@pytest.mark.parametrize("k", [1, 8, 64, 256])
def test_the_model_with_holes_is_the_reference(k):
    """Random levels and random holes (single ones, k apart, adjacent, in the first k frames, the last frame), six percentiles."""
    rng = np.random.default_rng(40 + k)
    panics = valid = 0
    for trial in range(12):
        t = int(rng.integers(8 * k + 2, 16 * k + 700))
        a = np.repeat(rng.integers(0, 9, t // 16 + 1), 16)[:t]
        holes = set(int(p) for p in rng.integers(0, t, int(rng.integers(0, 6))))
        if trial % 3 == 0:
            p = int(rng.integers(0, t - k - 1))
            holes |= {p, p + 1, p + k, t - 1, k - 1}
        frames = cases.hole_frames(a, sorted(holes), 4)
        var = npr.variance(frames, k)
        s, nan = cases.hole_sums(a, sorted(holes), k)
        assert np.array_equal(np.isnan(var), nan)
        assert np.array_equal(var[~nan] * np.float32(k), s[~nan].astype(np.float32))
        for perc in (0.0, 0.3, 0.5, 0.7, 0.9, 0.999):
            for min_len in (0, 7):
                want = reference(frames, k, perc, min_len)
                assert cases.hole_ranges(a, sorted(holes), k, cases.index_of(t, perc), min_len)[0] == want, (trial, perc, min_len)
                valid += want != "panic" and len(want) > 0
                panics += want == "panic"
    assert valid >= 30 and (panics > 0 or k == 1), (valid, panics)    # both outcomes are compared


def test_stretch_holes_cover_their_stretches_exactly():
    for k in (1, 8, 64):
        for stretches in ([(k, k + 64)], [(100 + k, 100 + 2 * k)], [(128, 131 + k), (300, 365 + k)], [(300, 811)]):
            a = np.ones(900, np.int64)
            assert cases.nan_columns(a, cases.stretch_holes(stretches, k), k) == stretches


# ---- every exact case against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.names("exact"))
def test_exact_cases_equal_the_reference(name):
    entry = cases.get(name)
    c = entry.case
    assert all(f.dtype == np.float32 and f.shape[1] == c.n_bins for f in c.recordings)
    assert c.k & (c.k - 1) == 0 and all(np.abs(np.asarray(a)).max() <= 8 for a, _ in entry.model)
    assert "wg" not in entry.facts or cases.workgroup(c.recordings) == entry.facts["wg"]
    want = [reference(f, c.k, c.perc, c.min_len) for f in c.recordings]
    assert entry.expected() == want
    panics = entry.facts.get("panics", [False] * len(want))
    assert [w == "panic" for w in want] == panics                 # no case panics unless it is named a panic
    builder, args = cases.BUILDERS[name]
    again = builder(*args)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again.case.recordings, c.recordings))


# ---- 1. the stretches ------------------------------------------------------------------------------------------------------------------
def geometry(shape, stretches, wg, k, t):
    """The stretches lie where the shape's name puts them."""
    lo, hi = stretches[0]
    step = lo // wg
    inside_one_step = all(l // wg == step and (h - 1) // wg == step for l, h in stretches)
    if shape.startswith("one wavefront"):
        j = (lo + 1) // WAVE                                        # the wavefront it covers (or is a column short of covering)
        d_lo, d_hi = lo - WAVE * j, hi - WAVE * (j + 1)
        moved = {"one wavefront": (0, 0), "one wavefront, a column short in front": (1, 0), "one wavefront, a column short behind": (0, -1),
                 "one wavefront, a column long in front": (-1, 0), "one wavefront, a column long behind": (0, 1)}[shape]
        # a wavefront inside its step: neither the first nor the last, so that the long ones stay within one step as well
        return len(stretches) == 1 and (d_lo, d_hi) == moved and 0 < j % (wg // WAVE) < wg // WAVE - 1 and inside_one_step
    if shape == "the first wavefront of a step":
        return len(stretches) == 1 and lo % wg == 0 and hi == lo + WAVE
    if shape == "the last wavefront of a step":
        return len(stretches) == 1 and hi % wg == 0 and hi == lo + WAVE
    if shape == "one step":
        return len(stretches) == 1 and lo % wg == 0 and hi == lo + wg
    if shape == "two steps and a part":
        return len(stretches) == 1 and lo % wg == 0 and 2 * wg < hi - lo < 3 * wg and hi % WAVE != 0
    if shape == "two wavefronts of a step":
        (l0, h0), (l1, h1) = stretches
        return inside_one_step and l0 % WAVE == 0 and h0 == l0 + WAVE and l1 % WAVE == 0 and h1 == l1 + WAVE and l1 - h0 >= WAVE and l0 % wg != 0
    if shape == "the last columns":
        return len(stretches) == 1 and hi == t and lo % WAVE != 0
    if shape == "from column k":
        return len(stretches) == 1 and lo == k and hi % WAVE == 0
    raise AssertionError(shape)


@pytest.mark.parametrize("name", cases.names("stretch"))
def test_stretches_lie_on_their_edges_and_a_range_spans_or_follows_them(name):
    entry = cases.get(name)
    c, facts = entry.case, entry.facts
    a, holes = entry.model[facts["main"]]
    t, wg, stretches, twin = len(a), facts["wg"], facts["stretches"], facts["twin"]
    assert t == len(c.recordings[facts["main"]]) and cases.workgroup(c.recordings) == wg and (t > cases.WG_SWITCH) == (wg == 1024)
    assert cases.nan_columns(a, holes, c.k) == stretches
    assert geometry(facts["shape"], stretches, wg, c.k, t), (name, stretches)
    if "one hole" in name:
        assert len(holes) == 1 and stretches[0][1] - stretches[0][0] == c.k
    ranges, _, open_at_end, th = cases.hole_ranges(a, holes, c.k, cases.index_of(t, c.perc), c.min_len)
    assert ranges != "panic" and 0 < th <= 8 * c.k
    lo, hi = stretches[0][0], stretches[-1][1]
    s, nan = cases.hole_sums(a, holes, c.k)
    between = [col for (_, h), (l, _) in zip(stretches[:-1], stretches[1:]) for col in range(h, l)]
    # no range begins or ends on an unclassified column, nor on one between two stretches
    assert not any(lo <= v < hi for r in ranges for v in r if v != hi)
    if twin == "open":
        assert s[lo - 1] >= th and all(s[col] >= th for col in between)
        if hi < t:
            spanning = [r for r in ranges if r[0] < lo and r[1] == hi]       # open across the stretch, closed by the first column behind
            assert len(spanning) == 1 and s[hi] < th
        else:
            assert open_at_end is not None and open_at_end < lo             # still open when the recording ends: never emitted
            assert not any(r[1] >= lo for r in ranges)
    else:
        assert s[lo - 1] < th and all(s[col] < th for col in between)
        assert not any(r[0] < lo <= r[1] for r in ranges)                    # nothing is open across the stretch
        if hi < t:
            following = [r for r in ranges if r[0] == hi]                    # opened by the first column behind
            assert len(following) == 1 and s[hi] >= th and following[0][1] - hi > c.min_len
        else:
            assert open_at_end is None
            assert not any(r[1] >= lo for r in ranges)


def test_every_shape_has_both_twins_at_both_workgroup_sizes():
    seen = {(e.facts["shape"], e.facts["twin"], e.facts["wg"]) for e in map(cases.get, cases.names("stretch"))}
    for wg in (256, 1024):
        for shape in cases.stretch_shapes(wg, 8):
            assert (shape, "idle", wg) in seen
            # the columns in front of column k are the literal zeros, below any positive threshold: no run is open across that stretch
            assert ((shape, "open", wg) in seen) == (shape != "from column k")


# ---- 2. dense emission -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.names("dense"))
def test_dense_cases_emit_exactly_the_bound_or_nothing(name):
    entry = cases.get(name)
    c, facts = entry.case, entry.facts
    assert c.k == 1 and cases.workgroup(c.recordings) == facts["wg"]
    assert (max(len(f) for f in c.recordings) > cases.WG_SWITCH) == (facts["wg"] == 1024)
    total = 0
    for (a, holes), m in zip(entry.model, facts["periods"]):
        t = len(a)
        assert not holes and t == 1 + m * facts["period"]
        ranges, short, open_at_end, th = cases.hole_ranges(a, [], 1, cases.index_of(t, c.perc), c.min_len)
        assert th == 5 and open_at_end is None
        if facts["barren"]:
            assert c.min_len == facts["period"] - 1 and ranges == [] and len(short) == m + 1    # the m periods and the run the scan starts in
            assert t // (c.min_len + 2) > 0                        # the device buffer is sized for ranges that never come
        else:
            assert c.min_len == facts["period"] - 2
            assert len(ranges) == m == t // (c.min_len + 2)         # the bound that sizes the device buffer, reached
            assert ranges[0] == (1, facts["period"]) and all(b - a_ == c.min_len + 1 for a_, b in ranges)
            if c.min_len == 0:
                assert [b for _, b in ranges] == list(range(2, t, 2))   # every other lane of every wavefront emits
        total += len(ranges)
    assert total == (0 if facts["barren"] else sum(facts["periods"]))


# ---- 3. the verdict boundary -------------------------------------------------------------------------------------------------------------
def test_verdict_cases_sit_on_the_boundary():
    entry = cases.get("verdict boundary")
    c, facts = entry.case, entry.facts
    idx = cases.index_of(cases.VERDICT_T, c.perc)
    assert idx == 500 and facts["nan"] == (498, 499, 500, 501)
    got = []
    for (a, holes), n_nan in zip(entry.model[1:-1], facts["nan"]):
        s, nan = cases.hole_sums(a, holes, c.k)
        assert len(a) == cases.VERDICT_T and int(nan.sum()) == n_nan
        ranges, _, _, th = cases.hole_ranges(a, holes, c.k, idx, c.min_len)
        classified = cases.VERDICT_T - n_nan
        assert (ranges == "panic") == (idx >= classified)
        if classified == idx + 1:
            assert th == s[~nan].max() and ranges                   # the last valid index: the threshold is the maximum
        got.append(classified - idx)
    assert got == [2, 1, 0, -1]
    assert entry.expected()[0] != "panic" and entry.expected()[-1] != "panic" and entry.expected()[-1]


# ---- 4. float cases ------------------------------------------------------------------------------------------------------------------------
def test_float_table_covers_the_stated_lengths_widths_and_windows():
    long_ones, wide_ones = set(), set()
    for name in cases.names("float"):
        c = cases.get(name).case
        if c.n_bins == 13 and len(c.recordings) == 2:
            long_ones.add((len(c.recordings[0]), c.k, cases.get(name).facts["dirty"]))
            assert len(c.recordings[1]) == 300
        else:
            assert tuple(len(f) for f in c.recordings) == (65, 257, 600)
            wide_ones.add((c.n_bins, c.k, cases.get(name).facts["dirty"]))
    assert long_ones == {(t, k, d) for t in (8191, 8192, 8193, 16385) for k in (15, 255, 257) for d in (False, True)}
    assert wide_ones == {(b, k, d) for b in (3, 47, 48, 49, 200) for k in (3, 200, 255, 256) for d in (False, True)}


@pytest.mark.parametrize("name", cases.names("float"))
def test_float_cases_do_not_panic_and_have_ranges(name):
    entry = cases.get(name)
    c = entry.case
    assert cases.workgroup(c.recordings) == entry.facts["wg"]
    want = [reference(f, c.k, c.perc, c.min_len) for f in c.recordings]
    assert "panic" not in want and any(want), name
    if entry.facts["dirty"]:
        with np.errstate(all="ignore"):
            var = [npr.variance(f, c.k) for f in c.recordings]
        assert any(np.isnan(v).any() for v in var) and any(np.isinf(v).any() for v in var)
        assert all(np.isnan(f).any() and (f == np.float32(1e30)).any() for f in c.recordings)
    else:
        assert all(np.isfinite(f).all() for f in c.recordings)
