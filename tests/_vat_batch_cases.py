"""The case table of the batched VAT edge tests ("Tests"): batches at which vat_variance_kernel,
vat_select_kernel and vat_scan_kernel (csrc/vat.hip) could leave the reference without tests/test_gpu_vat_batch.py noticing --
stretches of unclassified (NaN) columns laid on the scan's 64-column and workgroup-wide edges with a run open or idle across them,
recordings that emit as many ranges as the device buffer is sized for, the percentile's index on the last non-NaN variance and one
past it, and random frames at the lengths and widths where the kernels change path.  tests/test_vat_batch_cases.py shows on the CPU
that every case is what its name says; tests/test_gpu_vat_batch_edges.py runs every case on the device.  Pure numpy: the library is
not imported here, and a case is built only when it is asked for.

The exact cases extend the integer model of _companion_cases.integer_ranges to holes.  A hole is a frame of alternating(a) with one
bin set to NaN: its std is NaN, and so is the moving mean of every window that holds it -- columns p + 1 .. p + k for a hole at
frame p (the first k columns are the literal 0.0 whatever the frames are).  With k a power of two and |a| <= 8 every other mean,
std and moving mean is exact in f32, so k * variance[i] = sum |a[i - k:i]| in plain integers, the threshold is the idx-th smallest of
the classified sums, idx taken from the unfiltered length, and an idx at or past their number is the reference's panic."""
from collections import namedtuple

import numpy as np

import _companion_cases as cc

F = np.float32
WAVE = 64                      # columns per wavefront step of vat_scan_kernel
WG_SWITCH = 8192               # the longest recording of a batch up to which select and scan run 256 work-items, 1024 above
LENGTH = {256: 3000, 1024: 9000}

Case = namedtuple("Case", "recordings n_bins k perc min_len")


class Entry:
    """A case with what it claims.  kind: "exact" (model: per recording (a, holes), the answer is hole_ranges) or "float" (the answer
    is the oracle's).  facts: what the case is there to reach, checked by tests/test_vat_batch_cases.py."""

    def __init__(self, case, kind, model=None, **facts):
        self.case, self.kind, self.model, self.facts = case, kind, model, facts
        self._expected = None

    def expected(self):
        """Exact cases: per recording the model's ranges or "panic".  Computed once."""
        assert self.kind == "exact"
        if self._expected is None:
            c = self.case
            self._expected = [hole_ranges(a, holes, c.k, index_of(len(a), c.perc), c.min_len)[0] for a, holes in self.model]
        return self._expected


def workgroup(recordings):
    """Work-items per recording of vat_select_kernel and vat_scan_kernel for this batch."""
    return 256 if max(len(r) for r in recordings) <= WG_SWITCH else 1024


def index_of(t, perc):
    """numerics.rs:127-128: the f32 product, truncated."""
    return int(F(t) * F(perc))


# ---- the integer model with holes ---------------------------------------------------------------------------------------------------
def hole_sums(a, holes, k):
    """(k * variance as integers, unclassified?) per column, by prefix sums."""
    a = np.abs(np.asarray(a, np.int64))
    t = len(a)
    hole = np.zeros(t, np.int64)
    hole[list(holes)] = 1
    ca, ch = np.concatenate([[0], np.cumsum(a)]), np.concatenate([[0], np.cumsum(hole)])
    i = np.arange(t)
    lo = np.maximum(i - k, 0)
    return np.where(i >= k, ca[i] - ca[lo], 0), (i >= k) & (ch[i] - ch[lo] > 0)


def hole_ranges(a, holes, k, idx, min_len):
    """spectrogram.rs:192-216 on hole_frames(a, holes) in plain integers -> (emitted ranges or "panic", runs closed but too short,
    first column of the run still open at the end or None, the k-fold threshold)."""
    s, nan = hole_sums(a, holes, k)
    kept = np.sort(s[~nan])
    if idx >= len(kept):
        return "panic", [], None, None
    th = int(kept[idx])
    out, short, start, recording = [], [], 0, True
    for i, (v, n) in enumerate(zip(s.tolist(), nan.tolist())):
        if n:
            continue                                                # NaN >= th and NaN < th are both false
        if v >= th and not recording:
            start, recording = i, True
        if v < th and recording:
            recording = False
            (out if i - start > min_len else short).append((start, i))
    return out, short, (start if recording else None), th


def hole_frames(a, holes, n_bins):
    f = cc.alternating(a, n_bins)
    for p in holes:
        f[p, p % n_bins] = np.nan
    return f


def nan_columns(a, holes, k):
    """The maximal stretches [lo, hi) of unclassified columns."""
    nan = np.concatenate([[False], hole_sums(a, holes, k)[1], [False]])
    edges = np.flatnonzero(nan[1:] != nan[:-1])
    return [(int(lo), int(hi)) for lo, hi in zip(edges[::2], edges[1::2])]


def stretch_holes(stretches, k):
    """Holes at most k frames apart whose windows cover exactly the columns of every stretch [lo, hi): the first at lo - 1, the last
    at hi - k - 1."""
    holes = set()
    for lo, hi in stretches:
        assert hi - lo >= k and lo >= k
        holes.update(range(lo - 1, hi - k - 1, k))
        holes.add(hi - k - 1)
    return sorted(holes)


# ---- 1. stretches of unclassified columns on the scan's edges -------------------------------------------------------------------------
def neighbours():
    return list(cc.KAT_A), list(cc.random_integer_a())


def stretch_levels(t, k, stretches, twin, seed, pad):
    """32-frame levels in 0 .. 8 from the generator, and around the stretches levels set on purpose, (pad + 1) windows of each:
    `open`  ... 0s, 8s | stretch | 0s, 8s ...: a run opens on the 8s, is open across the stretch and closes on its first column behind;
    `idle`  ... 8s, 0s | stretch | 8s, 0s ...: a run closes on the 0s, none is open across the stretch, one opens on the first column
    behind and closes on the 0s that follow.  Between two stretches the level in front goes on."""
    a = np.repeat(np.random.default_rng(seed).integers(0, 9, t // 32 + 1), 32)[:t].copy()
    lo, hi = stretches[0][0], stretches[-1][1]
    front, behind = (8, 0) if twin == "open" else (0, 8)
    w = (pad + 1) * k
    if lo - 2 * w >= 0:
        a[lo - 2 * w:lo - w] = 8 - front
        a[lo - w:lo] = front
    else:
        assert lo == k and twin == "idle"                          # in front lie the k literal zeros and nothing else
    for (_, h), (l, _) in zip(stretches[:-1], stretches[1:]):
        a[h - k:l] = front
    if hi < t:
        assert hi + pad * k + w <= t
        a[hi - k:hi + pad * k] = behind
        a[hi + pad * k:hi + pad * k + w] = 8 - behind
    return a


def stretch_shapes(wg, k):
    """name -> stretches, for a batch whose scan runs `wg` work-items.  The step that holds them starts at column `base`."""
    t = LENGTH[wg]
    base = 4 * wg if wg == 256 else 3 * wg
    one = base + 2 * WAVE                                           # the third wavefront of the step
    behind = base + wg - (WAVE if wg == 256 else 2 * WAVE)          # the last wavefront of four, the last but one of sixteen
    return {
        "one wavefront": [(one, one + WAVE)],
        "one wavefront, a column short in front": [(one + 1, one + WAVE)],
        "one wavefront, a column short behind": [(one, one + WAVE - 1)],
        "one wavefront, a column long in front": [(one - 1, one + WAVE)],
        "one wavefront, a column long behind": [(one, one + WAVE + 1)],
        "the first wavefront of a step": [(base, base + WAVE)],
        "the last wavefront of a step": [(base + wg - WAVE, base + wg)],
        "one step": [(base, base + wg)],
        "two steps and a part": [(base, base + 2 * wg + wg // 4 + 5)],
        "two wavefronts of a step": [(base + WAVE, base + 2 * WAVE), (behind, behind + WAVE)],
        "the last columns": [(t - 100, t)],
        "from column k": [(k, 2 * WAVE)],
    }


def stretch_case(shape, twin, wg, k=8, pad=3):
    t = LENGTH[wg]
    stretches = stretch_shapes(wg, k)[shape]
    a = stretch_levels(t, k, stretches, twin, seed=1000 + wg + k, pad=pad)
    holes = stretch_holes(stretches, k)
    left, right = neighbours()
    model = [(left, []), (a, holes), (right, [])]
    case = Case([hole_frames(m, h, 4) for m, h in model], 4, k, 0.5, 5)
    return Entry(case, "exact", model, group="stretch", shape=shape, twin=twin, wg=wg, stretches=stretches, main=1)


# ---- 2. as many ranges as the device buffer is sized for ------------------------------------------------------------------------------
DENSE_PERC = 0.75


def dense_a(min_len, m):
    """k = 1: variance[i] = |a[i - 1]|.  m periods of (min_len + 1) 5s and a 1, and a last frame that no window reaches:
    t = 1 + m * (min_len + 2), and with the threshold 5 every period is a run of min_len + 1 columns, closed by its 1."""
    return np.concatenate([np.tile([5] * (min_len + 1) + [1], m), [1]])


def dense_case(min_len, wg, barren):
    """Three recordings; with wg = 1024 the middle one is longer than 8192 frames.  barren: min_len one larger than the period
    allows -- every run closes and none is emitted."""
    ms = (700, 333, 64) if wg == 256 else (700, WG_SWITCH // (min_len + 2) + 3, 333)
    model = [(dense_a(min_len, m), []) for m in ms]
    case = Case([hole_frames(a, [], 2) for a, _ in model], 2, 1, DENSE_PERC, min_len + 1 if barren else min_len)
    return Entry(case, "exact", model, group="dense", wg=wg, periods=ms, period=min_len + 2, barren=barren)


# ---- 3. the percentile's index on the last non-NaN variance, and past it --------------------------------------------------------------
VERDICT_T, VERDICT_K, VERDICT_NAN = 1000, 4, (498, 499, 500, 501)


def verdict_case():
    """perc = 0.5 of 1000 frames: index 500.  Recordings with 498, 499, 500 and 501 NaN columns between clean neighbours: 502 and 501
    classified columns are valid (with 501 the threshold is the maximum), 500 and 499 are the reference's panic."""
    a = np.repeat(np.random.default_rng(77).integers(0, 8, VERDICT_T // 32 + 1), 32)[:VERDICT_T].copy()
    a[100:200] = 8                                                  # the maximum, 4 * 8, on columns 104 .. 200: a run whatever the index
    left, right = neighbours()
    model = [(left, [])] + [(a, stretch_holes([(300, 300 + n)], VERDICT_K)) for n in VERDICT_NAN] + [(right, [])]
    case = Case([hole_frames(m, h, 4) for m, h in model], 4, VERDICT_K, 0.5, 5)
    return Entry(case, "exact", model, group="verdict", nan=VERDICT_NAN, panics=[False, False, False, True, True, False])


# ---- 4. random f32 frames where the kernels change path ------------------------------------------------------------------------------
def planted(rng, t, n_bins):
    """Random f32 frames with louder stretches, so that runs open and close at every length."""
    f = rng.standard_normal((t, n_bins)).astype(F)
    for lo, hi, g in ((t // 10, t // 4, 5.0), (t // 3, t // 3 + max(t // 40, 1), 9.0), (t // 2, (9 * t) // 10, 3.0)):
        f[lo:hi] *= F(g)
    return f


def spoil(f):
    """A frame with 1e30 in one bin (its std, and the k variances after it, are +inf) and a frame with a NaN."""
    t, n_bins = f.shape
    f[t // 5, 1 % n_bins] = 1e30
    f[t - 1 - t // 8, 0] = np.nan
    return f


FLOAT_LENGTHS, FLOAT_LONG_WINDOWS = (8191, 8192, 8193, 16385), (15, 255, 257)
FLOAT_WIDTHS, FLOAT_SHORT_LENGTHS, FLOAT_WIDE_WINDOWS = (3, 47, 48, 49, 200), (65, 257, 600), (3, 200, 255, 256)


def float_long_case(length, k, dirty):
    rng = np.random.default_rng(7000 + length + k)
    recs = [planted(rng, length, 13), planted(rng, 300, 13)]
    return Entry(Case([spoil(f) for f in recs] if dirty else recs, 13, k, 0.5, 5), "float", group="float", dirty=dirty,
                 wg=256 if length <= WG_SWITCH else 1024)


def float_wide_case(n_bins, k, dirty):
    rng = np.random.default_rng(8000 + 10 * n_bins + k)
    recs = [planted(rng, t, n_bins) for t in FLOAT_SHORT_LENGTHS]
    return Entry(Case([spoil(f) for f in recs] if dirty else recs, n_bins, k, 0.5, 5), "float", group="float", dirty=dirty, wg=256)


# ---- the table ----------------------------------------------------------------------------------------------------------------------
BUILDERS = {}


def _add(name, builder, *args):
    assert name not in BUILDERS
    BUILDERS[name] = (builder, args)


for _wg in (256, 1024):
    for _shape in stretch_shapes(_wg, 8):
        for _twin in ("open", "idle"):
            if _shape != "from column k" or _twin == "idle":       # in front of column k lie the literal zeros: no run is open there
                _add("%s, %s, %d work-items" % (_shape, _twin, _wg), stretch_case, _shape, _twin, _wg)
    for _twin in ("open", "idle"):
        # one hole and a window as long as the stretch
        _add("one wavefront, one hole, %s, %d work-items" % (_twin, _wg), stretch_case, "one wavefront", _twin, _wg, 64, 1)
for _twin in ("open", "idle"):
    _add("one step, one hole, %s, 256 work-items" % _twin, stretch_case, "one step", _twin, 256, 256, 1)
for _wg in (256, 1024):
    for _min_len in (0, 1, 2, 5):
        _add("dense, min_len %d, %d work-items" % (_min_len, _wg), dense_case, _min_len, _wg, False)
        _add("dense but a frame short, min_len %d, %d work-items" % (_min_len + 1, _wg), dense_case, _min_len, _wg, True)
_add("verdict boundary", verdict_case)
for _dirty in (False, True):
    for _length in FLOAT_LENGTHS:
        for _k in FLOAT_LONG_WINDOWS:
            _add("%d frames, window %d%s" % (_length, _k, ", non-finite" if _dirty else ""), float_long_case, _length, _k, _dirty)
    for _bins in FLOAT_WIDTHS:
        for _k in FLOAT_WIDE_WINDOWS:
            _add("%d bins, window %d%s" % (_bins, _k, ", non-finite" if _dirty else ""), float_wide_case, _bins, _k, _dirty)

_BUILT = {}


def names(group=None):
    return [n for n in BUILDERS if group is None or BUILDERS[n][0] in _GROUPS[group]]


_GROUPS = {"stretch": (stretch_case,), "dense": (dense_case,), "verdict": (verdict_case,), "float": (float_long_case, float_wide_case),
           "exact": (stretch_case, dense_case, verdict_case)}


def get(name):
    if name not in _BUILT:
        builder, args = BUILDERS[name]
        _BUILT[name] = builder(*args)
    return _BUILT[name]
