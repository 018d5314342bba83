"""The inputs of tests/test_gpu_spot_matrix.py, and the conditions they must meet, without a GPU: TEST INFRASTRUCTURE.

One case per spotting kernel <RT, D> that tests/_kernel_table.py reads from csrc/apd_internal.h (the sweep kind SpotSweep and the recording
kind SpotRecordSweep run the same case), and one per frame dimension of the <0, 0> group.  A case is a list of sequences of one
frame dimension, the (query, stream) pairs swept with unit penalties, the pairs swept with skewed ones, and -- for the kernels that
keep their rows in registers -- three pairs that send macro-steps down both square-root branches of csrc/dtw_spot_sweep.h (the
wave-wide gate `d2 >= 2^-96 and d2 < inf` on every squared distance of a macro-step, dead cells included).  What the kernels do
with a pair is restated here only as far as the inputs need it: which lane row holds query row n (kt.spot_row_n), and which
(query frame, stream frame) pairs one macro-step touches (macro_step_in_domain)."""
import collections
import zlib

import numpy as np

import _kernel_table as kt
import _path_reference as pref

F = np.float32
UNIT = (1.0, 1.0, 1.0)
SKEWED = (1.0, 2.0, 0.5)                        # (insertion, deletion, match)
STREAMS = (40, 91)                              # one below a wavefront, one above; one even, one odd: m + lane_n takes both parities
GATE_STREAM = 37
GATE_LOW, GATE_HIGH = F(2.0 ** -96), F(np.inf)  # sqrt_rn_finite's domain: [2^-96, inf)

Case = collections.namedtuple("Case", "kernel dim seqs lengths unit_pairs skewed_pairs gate_pairs tie_pairs")


def query_lengths(rt, register_rows):
    """The query lengths of row class rt.  Registers (rt = R >= 1): 64 (R - 1) + 1 and 64 R, and between them one length for every
    row of the lane that neither puts query row n on (R = 4: 193, 222, 231, 256).  LDS (rt = 0): the first length beyond the
    register classes, and one two rows per lane further."""
    if rt == 0:
        return [64 * register_rows + 1, 64 * (register_rows + 1) + 10]
    lo, hi = 64 * (rt - 1) + 1, 64 * rt
    lengths = [lo, hi]
    missing = [r for r in range(rt) if r not in {kt.spot_row_n(n)[1] for n in lengths}]
    for k, r in enumerate(missing):
        n = lo + 29 + 9 * k
        while kt.spot_row_n(n)[1] != r:
            n += 1
        assert lo < n < hi
        lengths.append(n)
    return sorted(lengths)


def any_dimensions(dims):
    """Source dimensions with no kernel dimension at or above them (<0, 0>): four consecutive ones, so that the squared-norm slot of
    the resident frame (float `dim` of ceil4(dim + 1)) falls in each float4 component, and one further up."""
    top = max(dims)
    return [top + 1, top + 2, top + 3, top + 4, top + 14]


def in_domain(sq):
    return (sq >= GATE_LOW) & (sq < GATE_HIGH)


def gate_sides(x, y):
    """(cells inside sqrt_rn_finite's domain, cells outside) among the live cells of the pair, by the checker's squared distances."""
    dom = in_domain(pref.sq_distances(x, y))
    return int(dom.sum()), int((~dom).sum())


def macro_step_in_domain(x, y, rt):
    """Per macro-step tau of spot_sweep<rt, D> on (x, y): True if every squared distance the wavefront computes in it -- lane l: its
    rt rows against column tau - l + 1; rows beyond n read query frame n, columns outside 1 .. m read stream frame m -- lies in
    the gate's domain.  The sweep takes its macro-steps two at a time: m + lane_n of them, rounded up to even."""
    n, m = len(x), len(y)
    assert kt.spot_rows_per_lane(n) == rt
    dom = in_domain(pref.sq_distances(x, y))
    rows = np.minimum(np.arange(64)[:, None] * rt + np.arange(rt)[None, :], n - 1)          # [lane][r], 0-based
    total = m + kt.spot_row_n(n)[0]
    out = []
    for tau in range(total + (total & 1)):
        col = tau - np.arange(64)
        col = np.where((col < 0) | (col >= m), m - 1, col)
        out.append(bool(dom[rows, col[:, None]].all()))
    return np.array(out)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _gate_pairs(rng, n, dim):
    """[(x, y)] * 3: plants, the lower edge of the domain, the upper edge."""
    m = GATE_STREAM
    x, y = rng.standard_normal((n, dim)).astype(F), rng.standard_normal((m, dim)).astype(F)
    cols = rng.choice(np.arange(1, m - 1), size=3, replace=False)                          # not the first, not the last stream frame
    rows = rng.choice(np.arange(0, n - 1), size=3, replace=False)                          # never the last query frame
    y[cols] = x[rows]
    out = [(x, y)]
    # Frames g * u * sqrt(8 / dim) * scale, g Gaussian: d2 of two frames is about 8 (u^2 + v^2) scale^2, times chi2_dim / dim.
    # The gate's edges are 16 * (2^-50)^2 = 2^-96 and 16 * (2^62)^2 = 2^128, so a pair of frames is inside for u^2 + v^2 > 2
    # (lower edge), < 2 (upper edge) -- up to the chi2 factor, which is what makes a column straddle.
    unit = np.sqrt(F(8.0) / F(dim)).astype(F)

    def frames(k, gain):
        return rng.standard_normal((k, dim)).astype(F) * gain.reshape(-1, 1).astype(F) * unit

    # lower edge: loud frames (u = 8) with four quiet ones (u = 0.7) in the query and in the stream: quiet against quiet falls below
    gx, gy = np.full(n, 8.0), np.full(m, 8.0)
    gx[rng.choice(np.arange(0, n - 1), size=4, replace=False)] = 0.7
    gy[rng.choice(np.arange(1, m - 1), size=4, replace=False)] = 0.7
    out.append((frames(n, gx) * F(2.0 ** -50), frames(m, gy) * F(2.0 ** -50)))
    # upper edge: quiet frames (u = 1 / 8); stream frame 2 overflows against every query frame (u = 4), stream frame 3 against some
    # (u = 1.3).  Only the stream: an overflowing query frame would leave +INF in every row below it.  Both columns have left the
    # wavefront after macro-step 65, and the sweep goes on for m + lane_n > 66 of them.
    gx, gy = np.full(n, 0.125), np.full(m, 0.125)
    gy[1], gy[2] = 4.0, 1.3
    out.append((frames(n, gx) * F(2.0 ** 62), frames(m, gy) * F(2.0 ** 62)))
    return out


def _build(kernel, dim, query_lens, skewed_len, gate_len, ties):
    rng = _rng("spot-matrix", kernel, dim)
    seqs = [rng.standard_normal((n, dim)).astype(F) for n in tuple(query_lens) + STREAMS]
    nq = len(query_lens)
    unit_pairs = [(q, nq + s) for q in range(nq) for s in range(len(STREAMS))]
    skewed_pairs = [(query_lens.index(skewed_len), nq + s) for s in range(len(STREAMS))]
    gate_pairs, tie_pairs = [], []
    if gate_len:
        for x, y in _gate_pairs(rng, gate_len, dim):
            gate_pairs.append((len(seqs), len(seqs) + 1))
            seqs += [x, y]
    if ties:
        tie_pairs.append((len(seqs), len(seqs) + 1))
        seqs += [rng.integers(0, 3, (65, dim)).astype(F), rng.integers(0, 3, (STREAMS[0], dim)).astype(F)]
    return Case(kernel, dim, seqs, [len(s) for s in seqs], unit_pairs, skewed_pairs, gate_pairs, tie_pairs)


_CASES = {}


def register_case(rt, d, register_rows=None):
    """The case of kernel <rt, d> at a kernel dimension d (the source dimension is d itself: nothing is padded)."""
    if (rt, d) not in _CASES:
        rows = kt.parse_spot_register_rows() if register_rows is None else register_rows
        lens = query_lengths(rt, rows)
        _CASES[(rt, d)] = _build((rt, d), d, lens, lens[-1], 64 * rt - 23 if rt else 0, False)
    return _CASES[(rt, d)]


def any_case(dim, dims=None, register_rows=None):
    """The case of source dimension dim in the <0, 0> group: queries of two row counts (the furthest dimension: R = 1 and
    R = kSpotRegisterRows + 2), and one pair of small integers, full of exact ties."""
    if (0, 0, dim) not in _CASES:
        dims = kt.parse_dims(kt.header_text()) if dims is None else dims
        rows = kt.parse_spot_register_rows() if register_rows is None else register_rows
        assert dim > max(dims)
        lens = [64, 64 * (rows + 1) + 10] if dim == any_dimensions(dims)[-1] else [65, 200]
        _CASES[(0, 0, dim)] = _build((0, 0), dim, lens, lens[-1], 0, True)
    return _CASES[(0, 0, dim)]


def register_kernels(text=None):
    return [k for k in kt.spot_kernels(text) if k[1] > 0]


def long_ends(m):
    return (1, 2, m // 2, m - 1, m)


def ends_of(m):
    """The ends asked of a stream of m frames: every column of the short one, five of the longer one."""
    return tuple(range(1, m + 1)) if m < 64 else long_ends(m)
