"""The table of degenerate alignment configurations that tests/test_config_cases.py (CPU) and tests/test_gpu_config_edges.py (GPU)
share: TEST INFRASTRUCTURE, no GPU, no code shared with the product.

include/apd.h accepts any f32 for the three penalties and for the band percentage, and any u64 for an explicit band
(oracle/apd_oracle.h, "the band's domain", is the definition the checkers follow).  An ENTRY is one such configuration with the
bound it is held to, by the rule the suite already has (tests/test_gpu_fuzz.py, BASELINE.json north_star):

  PARITY   positive finite EQUAL penalties: 1e-4 relative, identical zeros and +INF pattern (the fast distance forms);
  BITWISE  everything else -- a non-positive, infinite or NaN penalty (the literal kernel) and any unequal penalties (the literal
           select on strict distances): the oracle's bits, NaN payloads aside (_path_reference.bits).

No other number appears.  Strict mode is bitwise for every entry.  Subnormal penalties appear in an unequal entry only.

The batches are the smallest that reach the code: BATCH A (dim 13, 20 sequences: lengths 1, 2, 3, a spread of 30 .. 70, one of 130
-- more than one cell per lane of the literal kernel, three query rows per lane in spotting, a barycenter longer than a wavefront
--, an exact duplicate pair, an integer-valued pair; at 6.25 % the band binds for some pairs and |n-m| widens it for others),
BATCH B (A's sequences cut to dim 5, a dimension that is padded when made resident) and BATCH R (longest length 10, for the
f32-rounding percentage float32(0.7): the f32 product is exactly 7.0, the f64 product truncates to 6).
"""
import collections

import numpy as np

F = np.float32
INF, NAN = float("inf"), float("nan")
PARITY, BITWISE = "parity", "bitwise"
RTOL = 1e-4                                                      # BASELINE.json north_star, the PARITY bound

Entry = collections.namedtuple("Entry", "name pens pct bound")   # pens: (insertion, deletion, match)

# ---- penalties (insertion, deletion, match)
PENALTIES = [
    ("unit", (1.0, 1.0, 1.0)),
    ("ins0", (0.0, 1.0, 1.0)),
    ("del0", (1.0, 0.0, 1.0)),
    ("mat0", (1.0, 1.0, 0.0)),
    ("all0", (0.0, 0.0, 0.0)),
    ("ins-neg", (-0.5, 1.0, 1.0)),
    ("mat-neg", (1.0, 1.0, -2.0)),
    ("all-1", (-1.0, -1.0, -1.0)),
    ("ins-inf", (INF, 1.0, 1.0)),
    ("del-inf", (1.0, INF, 1.0)),
    ("mat-inf", (1.0, 1.0, INF)),
    ("all-inf", (INF, INF, INF)),
    ("ins-nan", (NAN, 1.0, 1.0)),
    ("del-nan", (1.0, NAN, 1.0)),
    ("mat-nan", (1.0, 1.0, NAN)),
    ("negzero", (-0.0, 1.0, 1.0)),
    ("all-negzero", (-0.0, -0.0, -0.0)),
    ("extremes", (2.0 ** -100, 1.0, 2.0 ** 100)),
    ("subnormal", (1e-44, 2e-44, 3e-44)),
    ("p2^60", (2.0 ** 60, 2.0 ** 60, 2.0 ** 60)),
    ("p2^-60", (2.0 ** -60, 2.0 ** -60, 2.0 ** -60)),
]
PENS = dict(PENALTIES)

# ---- band percentages.  SATURATED: the reference's band spans the whole matrix or overflows its usize: equal to pct = 1.0.
# VANISHING: the band is 0 (Rust's `as usize` of NaN, of a negative and of a product below 1): equal to pct = 0.0.
PCT_BINDS = 0.0625
PCT_SATURATED = [("pct1.5", 1.5), ("pct1e10", 1e10), ("pct1e30", 1e30), ("pct+inf", INF)]
PCT_VANISHING = [("pct-nan", NAN), ("pct-0.5", -0.5), ("pct-negzero", -0.0), ("pct0", 0.0), ("pct1e-9", 1e-9), ("pct-inf", -INF)]
PERCENTAGES = PCT_SATURATED + PCT_VANISHING
PCT_ROUNDING = float(F(0.7))                                     # x 10 frames: 7.0 in f32, 6.99999988 in f64

# ---- explicit bands of apd_align_pair (apd_alignment_params.warping_band, u64), beside 0 and max(n, m)
EXPLICIT_BANDS = [0, None, 2 ** 32 - 1, 2 ** 32, 0xFFFFFFF0, 2 ** 64 - 1]      # None: max(n, m) of the pair


def literal(pens):
    """choose_align_mode's `pens_ok` (csrc/apd_api.hip) negated: a penalty that is <= 0, infinite or NaN sends the call to the
    literal kernel (geometry 0)."""
    return not all(0.0 < p < INF for p in pens)


def bound_of(pens):
    equal = pens[0] == pens[1] == pens[2]
    return PARITY if (equal and not literal(pens)) else BITWISE


def _entry(pname, pct_name, pct):
    pens = PENS[pname]
    return Entry("%s/%s" % (pname, pct_name), pens, pct, bound_of(pens))


# every penalty set under the band that binds; every percentage under unit penalties (the fast kernels), a zero penalty (the
# literal kernel) and unequal ones (the literal select in the fast kernels)
PENALTY_ENTRIES = [_entry(p, "pct0.0625", PCT_BINDS) for p, _ in PENALTIES]
PERCENTAGE_ENTRIES = [_entry(p, n, v) for n, v in PERCENTAGES for p in ("unit", "ins0", "extremes")]
ENTRIES = PENALTY_ENTRIES + PERCENTAGE_ENTRIES + [_entry("unit", "pct1", 1.0), _entry("ins0", "pct1", 1.0), _entry("extremes", "pct1", 1.0)]
BY_NAME = {e.name: e for e in ENTRIES}
assert len(BY_NAME) == len(ENTRIES)

# the f32-rounding case runs on batch R under a negative deletion penalty: with non-negative penalties the one cell that band 7
# adds to band 6 in a 10 x 10 table -- (1, 9) -- can never be the smaller predecessor of (2, 9), so no score could tell the bands apart
ROUNDING_ENTRY = Entry("del-neg/pct-f32(0.7)", (1.0, -1.0, 1.0), PCT_ROUNDING, BITWISE)

LENGTHS_A = [1, 2, 3, 30, 33, 37, 41, 45, 48, 52, 52, 57, 61, 64, 66, 70, 40, 40, 130, 35]
DUP_A = (9, 10)                                                  # sequence 10 is an exact copy of sequence 9
INTEGER_A = (16, 17)                                             # small integers: exact ties in the select
LONG_A = 18
LENGTHS_R = [10, 10, 10, 7, 4, 9]

Batch = collections.namedtuple("Batch", "key dim seqs frames offsets lens")
_batches = {}


def _pack(key, seqs):
    seqs = [np.ascontiguousarray(s, dtype=F) for s in seqs]
    offsets = np.zeros(len(seqs) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    return Batch(key, seqs[0].shape[1], seqs, np.concatenate(seqs, axis=0), offsets, [len(s) for s in seqs])


def batch(key):
    """"A", "B" or "R"; built once."""
    if key in _batches:
        return _batches[key]
    if key == "A":
        rng = np.random.default_rng(20250)
        # one random walk of 130 frames; every other sequence reads it through a time warp of its own (t / n) ** g plus a little
        # noise, so that the cheapest path between two of them strays far from the diagonal and the band decides scores
        base = np.cumsum(rng.standard_normal((130, 13)), axis=0) * 0.4
        seqs = []
        for k, n in enumerate(LENGTHS_A):
            g = (0.45, 0.7, 1.0, 1.5, 2.2)[k % 5]
            t = np.floor(129.0 * (np.arange(n) / max(n - 1, 1)) ** g).astype(np.int64)
            seqs.append((base[t] + 0.05 * rng.standard_normal((n, 13))).astype(F))
        seqs[DUP_A[1]] = seqs[DUP_A[0]].copy()
        for s in INTEGER_A:
            seqs[s] = rng.integers(-2, 3, (LENGTHS_A[s], 13)).astype(F)
        out = _pack("A", seqs)
    elif key == "B":
        out = _pack("B", [s[:, :5].copy() for s in batch("A").seqs])
    elif key == "R":
        rng = np.random.default_rng(707)
        out = _pack("R", [rng.standard_normal((n, 13)).astype(F) * F(3.0) for n in LENGTHS_R])
    else:
        raise KeyError(key)
    _batches[key] = out
    return out


# The pairs of batch A that the per-cell Python checkers (np_reference, _path_reference) walk: the one-, two- and three-frame
# sequences against each other and against a long one, a pair whose band binds at 6.25 % (64 vs 66: band 4, gap 2), one that
# |n-m| widens (30 vs 37: band 2, gap 7), the duplicate pair, the integer pair; both orders of each.
_SLOW = [(0, 1), (0, 2), (1, 2), (0, 3), (2, 4), (3, 5), (13, 14), DUP_A, INTEGER_A, (19, 3)]
SLOW_PAIRS = _SLOW + [(b, a) for a, b in _SLOW]


def same_bits(got, want):
    """Bitwise equality of two f32 arrays, every NaN one pattern (_path_reference.bits)."""
    from _path_reference import bits
    return np.array_equal(bits(got), bits(want))


def check(got, want, bound, what=""):
    """The entry's bound.  BITWISE: the bits, NaN payloads aside.  PARITY: 1e-4 relative with identical zeros, NaN and +-INF
    pattern."""
    from _path_reference import bits
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, what
    if bound == BITWISE:
        differing = int((bits(got) != bits(want)).sum())
        assert differing == 0, "%s: %d of %d entries differ bitwise from the checker" % (what, differing, got.size)
        return
    assert bound == PARITY
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got)), what + ": INF/NaN pattern differs"
    assert np.array_equal(np.isposinf(want), np.isposinf(got)) and np.array_equal(np.isnan(want), np.isnan(got)), what
    zero = fin & (want == 0)
    assert np.all(got[zero] == 0), what + ": exact zeros must stay 0"
    nz = fin & ~zero
    if nz.any():
        rel = float((np.abs(got[nz].astype(np.float64) - want[nz]) / np.abs(want[nz].astype(np.float64))).max())
        assert rel <= RTOL, "%s: max rel err %.3e" % (what, rel)


_wants = {}


def want_matrix(oracle, key, entry):
    """The oracle's matrix of batch `key` under `entry`, computed once and handed out read-only."""
    k = (key, entry.name)
    if k not in _wants:
        b = batch(key)
        m = oracle.align_all(b.frames, b.offsets, entry.pct, *entry.pens, workers=4)
        m.setflags(write=False)
        _wants[k] = m
    return _wants[k]
