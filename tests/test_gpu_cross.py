"""apd_batch_join + apd_align_cross: one set of sequences aligned against another, against the CPU oracle.

"Oracle" is oracle.align_sample on the concatenation first + second: pairs (q, n1 + c) give fs[q][c], pairs (n1 + c, q) give sf[c][q].
"Bitwise" is equality as uint32; "parity" the rule of tests/test_gpu_dtw.py::assert_parity (same 0 / +INF pattern, <= 1e-4 relative),
copied below.  Bounds: strict mode, the literal kernel (set_variant(1)) and unequal penalties are bitwise, everything else parity --
per kernel family as tests/test_gpu_kernel_matrix.py's FORMS table has them.  Seeds are fixed.  No default-mode case needed the
coincidental-tie rule of DESIGN.md section 6: none is re-seeded.

A cross tile holds pairs whose column sequence `a` may be the SHORTER one (in a length-ordered batch it never is): the family test
forces every kernel family through cross tiles with the first set strictly shorter, strictly longer, and interleaved.
"""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import _kernel_table as kt
import _path_reference as pr

pytestmark = pytest.mark.gpu
RTOL = 1e-4
UNIT, EQUAL, UNEQUAL = (1.0, 1.0, 1.0), (0.7, 0.7, 0.7), (0.6, 1.3, 1.0)
F32P = C.POINTER(C.c_float)


def assert_parity(got, want, what=""):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got)), what + ": INF/NaN pattern differs"
    assert np.array_equal(np.isposinf(want), np.isposinf(got)), what
    zero = fin & (want == 0)
    assert np.all(got[zero] == 0), what + ": exact zeros must stay 0"
    nz = fin & ~zero
    if nz.any():
        rel = np.abs(got[nz] - want[nz]) / np.abs(want[nz])
        print("%s: max rel err %.3e over %d entries" % (what, rel.max(), int(nz.sum())))
        assert rel.max() <= RTOL, "%s: max rel err %.3e" % (what, rel.max())


def assert_bitwise(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape
    differing = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print("%s: %d of %d entries differ bitwise" % (what, differing, got.size))
    assert differing == 0, "%s: %d of %d entries differ bitwise from the oracle" % (what, differing, got.size)


def check(got, want, bitwise, what):
    (assert_bitwise if bitwise else assert_parity)(got, want, what)


def walks(key, lens, dim):
    """Random-walk sequences of the given lengths (the generator of tests/test_gpu_kernel_matrix.py)."""
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    return [np.cumsum(rng.standard_normal((int(n), dim)), axis=0).astype(np.float32) * np.float32(0.4) for n in lens]


def pack(seqs, dim):
    offsets = np.zeros(len(seqs) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    frames = np.concatenate(seqs, axis=0) if seqs else np.zeros((0, dim), np.float32)
    return np.ascontiguousarray(frames, np.float32).reshape(-1, dim), offsets


_wants = {}


def oracle_cross(oracle, key, A, B, dim, pct, pens=UNIT):
    """(fs [n1][n2], sf [n2][n1]) of the oracle, cached per key."""
    k = (key, pct, pens)
    if k not in _wants:
        n1, n2 = len(A), len(B)
        frames, offsets = pack(A + B, dim)
        q, c = np.meshgrid(np.arange(n1), np.arange(n2), indexing="ij")
        fs = oracle.align_sample(frames, offsets, q.ravel(), n1 + c.ravel(), pct, *pens, workers=8)[0].reshape(n1, n2)
        sf = oracle.align_sample(frames, offsets, n1 + c.T.ravel(), q.T.ravel(), pct, *pens, workers=8)[0].reshape(n2, n1)
        _wants[k] = (fs, sf)
    return _wants[k]


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    c.set_distance_mode("hybrid")
    yield c
    c.set_variant(0)
    c.close()


class Joined:
    """Two resident batches and their join."""

    def __init__(self, ctx, A, B, dim):
        from audio_pattern_discovery_amd.alignments import Batch
        self.ctx, self.n1, self.n2 = ctx, len(A), len(B)
        self.a = Batch(ctx, *pack(A, dim), dim)
        self.b = Batch(ctx, *pack(B, dim), dim)
        self.j = Batch.join(self.a, self.b)

    def cross(self, cfg, fs=True, sf=True):
        from audio_pattern_discovery_amd import _lib
        out_fs = np.full((self.n1, self.n2), -7.0, np.float32) if fs else None
        out_sf = np.full((self.n2, self.n1), -7.0, np.float32) if sf else None
        rc = _lib.lib().apd_align_cross(self.ctx.handle, self.j.handle, C.byref(cfg), out_fs.ctypes.data_as(F32P) if fs else None,
                                        out_sf.ctypes.data_as(F32P) if sf else None)
        return rc, out_fs, out_sf

    def close(self):
        for b in (self.j, self.b, self.a):
            b.close()


def config(pct, pens=UNIT):
    from audio_pattern_discovery_amd.discovery import Discovery
    return Discovery(warping_band_percentage=pct, insertion_penalty=pens[0], deletion_penalty=pens[1], match_penalty=pens[2]).align_config()


def run_cross(ctx, A, B, dim, pct, pens=UNIT, mode="hybrid", variant=0, capfd=None, fs=True, sf=True):
    """(fs, sf, {geometry code: tiles}) of one cross alignment; APD_OK asserted."""
    ctx.set_distance_mode(mode)
    ctx.set_variant(variant)
    plan = None
    if capfd is not None:
        os.environ["APD_DEBUG_PLAN"] = "1"
        capfd.readouterr()
    try:
        j = Joined(ctx, A, B, dim)
        rc, out_fs, out_sf = j.cross(config(pct, pens), fs, sf)
        j.close()
        if capfd is not None:
            plan = kt.read_plan(capfd.readouterr().err)
    finally:
        os.environ.pop("APD_DEBUG_PLAN", None)
        ctx.set_variant(0)
        ctx.set_distance_mode("hybrid")
    assert rc == 0, rc
    return out_fs, out_sf, plan


def ragged(key, n1, n2, dim, lo=37, hi=67):
    rng = np.random.default_rng(zlib.crc32(repr(("lens",) + key).encode()))
    lens = rng.integers(lo, hi + 1, size=n1 + n2)
    seqs = walks(key, lens, dim)
    return seqs[:n1], seqs[n1:]


MODES = [("strict", "strict", 0, True), ("literal", "hybrid", 1, True), ("default", "hybrid", 0, False)]
SHAPES = [(21, 37), (5, 40), (16, 32), (32, 16), (1, 1), (1, 20), (17, 1)]


# ---- 1. shapes of the rectangle

@pytest.mark.parametrize("n1,n2", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_rectangle_shapes_match_the_oracle(ctx, oracle, n1, n2):
    """A straddling diagonal tile (21, 37), a straddle inside tile (0, 0) (5, 40), no straddle (16, 32) / (32, 16), single sequences,
    several tile rows on either side.  Both outputs, then each alone with the other NULL."""
    A, B = ragged(("shape", n1, n2), n1, n2, 13)
    want_fs, want_sf = oracle_cross(oracle, ("shape", n1, n2), A, B, 13, 0.0625)
    for name, mode, variant, bitwise in MODES:
        fs, sf, _ = run_cross(ctx, A, B, 13, 0.0625, UNIT, mode, variant)
        check(fs, want_fs, bitwise, "%s fs" % name)
        check(sf, want_sf, bitwise, "%s sf" % name)
        fs1, none, _ = run_cross(ctx, A, B, 13, 0.0625, UNIT, mode, variant, sf=False)
        assert none is None and np.array_equal(fs1.view(np.uint32), fs.view(np.uint32)), name + ": fs alone differs from fs of the pair"
        none, sf1, _ = run_cross(ctx, A, B, 13, 0.0625, UNIT, mode, variant, fs=False)
        assert none is None and np.array_equal(sf1.view(np.uint32), sf.view(np.uint32)), name + ": sf alone differs from sf of the pair"


# ---- 2. planes are not swapped

def test_planes_are_not_swapped(ctx, oracle):
    """Under unequal penalties score(x, y) != score(y, x) for nearly every pair, so a kernel or an unpack that exchanged the two slab
    planes fails; with unit penalties only about one entry in a hundred would notice."""
    pens = (1.5, 0.75, 1.25)
    A, B = ragged(("planes",), 21, 37, 13)
    want_fs, want_sf = oracle_cross(oracle, ("planes",), A, B, 13, 0.0625, pens)
    share = float((want_fs != want_sf.T).mean())
    print("oracle: fs != sf.T in %.1f %% of the entries" % (100 * share))
    assert share > 0.9
    for name, mode, variant, _ in MODES:                        # non-unit penalties: the literal arithmetic in every mode
        fs, sf, _ = run_cross(ctx, A, B, 13, 0.0625, pens, mode, variant)
        assert_bitwise(fs, want_fs, name + " fs")
        assert_bitwise(sf, want_sf, name + " sf")


# ---- 3. swap symmetry

def test_join_order_does_not_matter(ctx, oracle):
    """join(A, B) and join(B, A) hold the same pairs with the sets' roles exchanged: fs of one is sf of the other."""
    A, B = ragged(("swap",), 21, 37, 13)
    want_fs, want_sf = oracle_cross(oracle, ("swap",), A, B, 13, 0.0625)
    for name, mode, variant, bitwise in MODES:
        fs, sf, _ = run_cross(ctx, A, B, 13, 0.0625, UNIT, mode, variant)
        fs_r, sf_r, _ = run_cross(ctx, B, A, 13, 0.0625, UNIT, mode, variant)      # fs_r[c][q] = score(x = B c, y = A q) = sf[c][q]
        if bitwise:
            assert np.array_equal(fs.view(np.uint32), sf_r.view(np.uint32)) and np.array_equal(sf.view(np.uint32), fs_r.view(np.uint32)), name
        for got, want, what in ((fs, want_fs, "fs"), (sf, want_sf, "sf"), (sf_r, want_fs, "sf of the reverse join"),
                                (fs_r, want_sf, "fs of the reverse join")):
            check(got, want, bitwise, "%s %s" % (name, what))


# ---- 4. every kernel family, both orientations

# family -> (forced code, [(form, penalties, distance mode, bitwise)]): the forms of tests/test_gpu_kernel_matrix.py's FORMS table;
# the generic kernel is the literal one: bitwise in every form
FAMILIES = {
    "systolic": (kt.encode("systolic", 16, 9), [("unit-hybrid", UNIT, "hybrid", False), ("unit-exact", UNIT, "exact", False),
                                                ("unit-strict", UNIT, "strict", True), ("unequal", UNEQUAL, "hybrid", True)]),
    "shared": (kt.encode("shared", 16, 9), [("unit-hybrid", UNIT, "hybrid", False)]),
    "strip": (kt.encode("strip", 4, 5), [("unit-hybrid", UNIT, "hybrid", False), ("unit-exact", UNIT, "exact", False),
                                         ("p07-hybrid", EQUAL, "hybrid", False), ("p07-exact", EQUAL, "exact", False)]),
    "banded": (kt.encode("banded", 4, 5), [("unit-hybrid", UNIT, "hybrid", False), ("unit-exact", UNIT, "exact", False),
                                           ("p07-exact", EQUAL, "exact", False), ("unequal", UNEQUAL, "hybrid", True),
                                           ("unit-strict", UNIT, "strict", True)]),
    "wide": (kt.encode("wide", 2, 5), [("unit-hybrid", UNIT, "hybrid", False), ("unit-exact", UNIT, "exact", False),
                                       ("p07-hybrid", EQUAL, "hybrid", False), ("p07-exact", EQUAL, "exact", False)]),
    "generic": (1, [("unit-hybrid", UNIT, "hybrid", True), ("unequal", UNEQUAL, "hybrid", True)]),
}


def family_lengths(fam):
    """(16 long lengths, 21 short lengths, band percentage) such that the forced code of `fam` accepts every tile whose two rows hold
    any of them (plan_tile_classes, csrc/dtw_generic.hip); every short length is below every long one; 1, 2 and 3 are among the
    short ones.  The long set fills exactly one tile row, so the rectangle is tiles (0, 1) and (0, 2).
    systolic / generic: 2w + 1 <= 144 with w <= 68 - 1 + 2.  shared: the spread of w inside a tile stays within the ring's slack of
    19 (w between 24 and 41).  strip: a full band.  banded: the band binds (90 %) and every tile row holds a sequence of 50 frames
    or more (the 17 longest short ones).  wide: 2w + 1 <= 640 with w <= 300 - 1 + 2."""
    if fam in ("systolic", "generic"):
        return [68 - k % 9 for k in range(16)], [30 - k for k in range(18)] + [3, 2, 1], 0.5
    if fam == "shared":
        return [40 - k % 7 for k in range(16)], [12 - k % 9 for k in range(18)] + [3, 2, 1], 0.5
    if fam == "strip":
        return [170 - 4 * k for k in range(16)], [90 - 4 * k for k in range(18)] + [3, 2, 1], 1.0
    if fam == "banded":
        return [170 - 4 * k for k in range(16)], [84 - 2 * k for k in range(17)] + [3, 2, 1, 2], 0.9
    assert fam == "wide"
    return [300 - 6 * k for k in range(16)], [150 - 7 * k for k in range(18)] + [3, 2, 1], 0.3


def family_sets(fam, arrangement, dim=13):
    """(first set, second set, band percentage) of one family test."""
    long_, short, pct = family_lengths(fam)
    assert max(short) < min(long_) and {1, 2, 3} <= set(short)
    if arrangement == "first-shorter":
        la, lb = short, long_
    elif arrangement == "first-longer":
        la, lb = long_, short
    else:
        # interleaved: both orientations inside one tile.  The shared-column rule bounds the spread of w per workgroup, which
        # short-short pairs next to long-short ones would exceed: that family keeps every length within 19 frames.
        pool = long_ + short if fam != "shared" else [19 - k % 7 for k in range(16)] + [12 - k % 9 for k in range(18)] + [3, 2, 1]
        desc = sorted(pool, reverse=True)
        la, lb = desc[0::2][:16], desc[1::2] + desc[0::2][16:]      # alternate ranks: the first set keeps 16 members and the larger mean
        assert sum(la) * len(lb) > sum(lb) * len(la) and {1, 2, 3} <= set(lb)
        if fam == "banded":                                         # every tile row of the second set needs a sequence of >= 50 frames
            assert sorted(lb, reverse=True)[16] >= 50
    assert (len(la), len(lb)) in ((16, 21), (21, 16))
    A, B = walks((fam, arrangement, "a"), la, dim), walks((fam, arrangement, "b"), lb, dim)
    if arrangement == "interleaved":                                # one exact copy across the sets (the longest of each): 0.0 both ways
        B[max(range(len(B)), key=lambda s: len(B[s]))] = max(A, key=len).copy()
    return A, B, pct


FAMILY_CASES = [(fam, arr) for fam in FAMILIES for arr in ("first-shorter", "first-longer", "interleaved")]


@pytest.mark.parametrize("fam,arrangement", FAMILY_CASES, ids=["%s-%s" % c for c in FAMILY_CASES])
def test_every_kernel_family_sweeps_cross_tiles_in_both_orientations(ctx, oracle, capfd, fam, arrangement):
    code, forms = FAMILIES[fam]
    A, B, pct = family_sets(fam, arrangement)
    la, lb = [len(s) for s in A], [len(s) for s in B]
    if arrangement == "first-shorter":
        assert max(la) < min(lb)
    elif arrangement == "first-longer":
        assert min(la) > max(lb)
    else:
        longer_a = sum(1 for x in la for y in lb if x > y)
        assert 0.2 < longer_a / (len(la) * len(lb)) < 0.8          # both orientations occur
    copies = [(q, c) for q in range(len(A)) for c in range(len(B)) if A[q].shape == B[c].shape and np.array_equal(A[q], B[c])]
    assert (len(copies) >= 1) == (arrangement == "interleaved")
    n_tiles = 2                                                     # one tile row of 16 against 21 sequences: tiles (0, 1) and (0, 2)
    for name, pens, mode, bitwise in forms:
        want_fs, want_sf = oracle_cross(oracle, (fam, arrangement), A, B, 13, pct, pens)
        for q, c in copies:
            assert want_fs[q, c] == 0.0 and want_sf[c, q] == 0.0
        fs, sf, plan = run_cross(ctx, A, B, 13, pct, pens, mode, code, capfd)
        expect = {0: n_tiles} if fam == "generic" else {code: n_tiles}
        assert plan == expect, "%s %s %s: the plan is %r, not every cross tile on %d" % (fam, arrangement, name, plan, code)
        check(fs, want_fs, bitwise, "%s %s %s fs" % (fam, arrangement, name))
        check(sf, want_sf, bitwise, "%s %s %s sf" % (fam, arrangement, name))


# ---- 5. the joined batch as an ordinary batch

def test_joined_batch_is_an_ordinary_batch(ctx, oracle, apd):
    from audio_pattern_discovery_amd.alignments import Batch, PATH_STEP
    L = apd.lib()
    n1, n2, dim = 21, 37, 13
    A, B = ragged(("ordinary",), n1, n2, dim)
    n = n1 + n2
    frames, offsets = pack(A + B, dim)
    j = Joined(ctx, A, B, dim)
    assert L.apd_batch_len(j.j.handle) == n and L.apd_batch_first_len(j.j.handle) == n1 and j.j.first_len() == n1
    assert L.apd_batch_first_len(j.a.handle) == n1                  # a plain batch: all of it
    cfg = config(0.0625)
    ctx.set_distance_mode("strict")
    try:
        full = np.zeros((n, n), np.float32)
        apd.check(L.apd_align_all(ctx.handle, j.j.handle, C.byref(cfg), full.ctypes.data_as(F32P)), ctx.handle)
        rc, fs, sf = j.cross(cfg)
        assert rc == 0
    finally:
        ctx.set_distance_mode("hybrid")
    assert_bitwise(full, oracle.align_all(frames, offsets, 0.0625, workers=8), "align_all on the joined batch")
    assert np.array_equal(full[:n1, n1:].view(np.uint32), fs.view(np.uint32)) and np.array_equal(full[n1:, :n1].view(np.uint32), sf.view(np.uint32))
    # warping paths between a query and a corpus item
    pairs = np.array([(0, n1 + 5), (20, n1), (7, n - 1)], np.uint32)
    off = np.zeros(4, np.uint64)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    apd.check(L.apd_align_paths(ctx.handle, j.j.handle, C.byref(cfg), pairs.ctypes.data_as(u32p), 3, None, 0, off.ctypes.data_as(u64p), None, None),
              ctx.handle)
    steps, lens, scores = np.zeros(int(off[-1]), PATH_STEP), np.zeros(3, np.uint32), np.zeros(3, np.float32)
    apd.check(L.apd_align_paths(ctx.handle, j.j.handle, C.byref(cfg), pairs.ctypes.data_as(u32p), 3, steps.ctypes.data_as(C.POINTER(apd.PathStep)),
                                len(steps), off.ctypes.data_as(u64p), lens.ctypes.data_as(u32p), scores.ctypes.data_as(F32P)), ctx.handle)
    seqs = A + B
    for p, (x, y) in enumerate(pairs):
        band = oracle.warping_band(0.0625, max(len(seqs[x]), len(seqs[y])))
        want_steps, want_score = pr.path(seqs[x], seqs[y], band)
        got = steps[int(off[p]):int(off[p]) + int(lens[p])]
        assert len(got) == len(want_steps)
        for name in ("i", "j", "op"):
            assert np.array_equal(got[name], want_steps[name]), (p, name)
        assert np.array_equal(got["cost"].view(np.uint32), want_steps["cost"].view(np.uint32)), p
        assert np.float32(scores[p]).view(np.uint32) == np.float32(want_score).view(np.uint32)
        assert np.float32(scores[p]).view(np.uint32) == fs[x, y - n1].view(np.uint32)
    # refusals
    assert L.apd_batch_refill(ctx.handle, j.j.handle, C.c_void_p(frames.ctypes.data), 0) == apd.APD_ERR_INVALID_ARG
    out = np.zeros((n1, n2), np.float32)
    assert L.apd_align_cross(ctx.handle, j.a.handle, C.byref(cfg), out.ctypes.data_as(F32P), None) == apd.APD_ERR_INVALID_ARG
    other = apd.Context(0)
    try:
        foreign = Batch(other, *pack(B, dim), dim)
        h = C.c_void_p()
        assert L.apd_batch_join(ctx.handle, j.a.handle, foreign.handle, C.byref(h)) == apd.APD_ERR_INVALID_ARG and not h.value
        foreign.close()
    finally:
        other.close()
    narrow = Batch(ctx, *pack(walks(("dim8",), [40, 50], 8), 8), 8)
    h = C.c_void_p()
    assert L.apd_batch_join(ctx.handle, j.a.handle, narrow.handle, C.byref(h)) == apd.APD_ERR_INVALID_ARG and not h.value
    narrow.close()
    j.close()


# ---- 6. feature range

@pytest.mark.parametrize("where", ["second", "first", "neither"])
def test_feature_range_follows_both_sets(ctx, oracle, apd, where):
    n1, n2, dim = 21, 37, 13
    A, B = ragged(("range",), n1, n2, dim)
    A, B = [s.copy() for s in A], [s.copy() for s in B]
    if where != "neither":
        odd = B if where == "second" else A
        odd[3][5, 2] = np.inf
        odd[9][0, 7] = np.float32(1e-42)
    want_fs, want_sf = oracle_cross(oracle, ("range", where), A, B, dim, 0.0625)
    if where != "neither":
        assert np.isposinf(want_fs).any() or np.isnan(want_fs).any()
    j = Joined(ctx, A, B, dim)
    nf = C.c_int(-1)
    apd.check(apd.lib().apd_batch_nonfinite(ctx.handle, j.j.handle, C.byref(nf)), ctx.handle)
    j.close()
    assert nf.value == (0 if where == "neither" else 1)
    if where == "neither":
        return
    for name, mode, variant, _ in MODES + [("exact", "exact", 0, True)]:
        fs, sf, _ = run_cross(ctx, A, B, dim, 0.0625, UNIT, mode, variant)
        same = lambda g, w: np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~np.isnan(w)].view(np.uint32), w[~np.isnan(w)].view(np.uint32))
        assert same(fs, want_fs) and same(sf, want_sf), name + ": not the oracle's bits (NaN payloads aside)"
        assert np.array_equal(np.isposinf(fs), np.isposinf(want_fs))


# ---- 7. poison

def resident_positions(la, lb):
    """(swapped, first resident segment, second): each segment the sequence numbers of one set in its length order (longest first,
    equal lengths by ascending index); the set with the larger mean length lies first, the first set on a tie."""
    order = lambda lens: sorted(range(len(lens)), key=lambda s: (-lens[s], s))
    swapped = sum(la) * len(lb) < sum(lb) * len(la)
    return (swapped, order(lb), order(la)) if swapped else (swapped, order(la), order(lb))


def test_a_shortened_cross_launch_is_reported_not_zero_filled(ctx, oracle, apd, capfd):
    n1, n2, dim = 21, 37, 13
    A, B = ragged(("poison",), n1, n2, dim)
    want_fs, want_sf = oracle_cross(oracle, ("poison",), A, B, dim, 0.0625)
    cfg = config(0.0625)
    j = Joined(ctx, A, B, dim)
    os.environ["APD_DEBUG_PLAN"] = "1"
    capfd.readouterr()
    # the hook drops the last tile of EVERY kernel class: with the literal kernel forced there is one class, the whole rectangle,
    # and the dropped tile is the rectangle's last one (the automatic plan splits these lengths over three geometries)
    ctx.set_variant(1)
    ctx.set_fault_injection(1)
    try:
        rc, fs, sf = j.cross(cfg)
    finally:
        ctx.set_fault_injection(0)
        ctx.set_variant(0)
        os.environ.pop("APD_DEBUG_PLAN", None)
    plan = kt.read_plan(capfd.readouterr().err)
    assert rc == apd.APD_ERR_INCOMPLETE
    assert list(plan) == [0] and plan[0] == 6, plan                   # tiles (0, 1) .. (0, 3), (1, 1) .. (1, 3)
    swapped, seg0, seg1 = resident_positions([len(s) for s in A], [len(s) for s in B])
    n0, n = len(seg0), n1 + n2
    ta, tb = (n0 + 15) // 16 - 1, (n + 15) // 16 - 1                 # the last tile of the rectangle
    rows = [seg0[p] for p in range(ta * 16, min(ta * 16 + 16, n0))]
    cols = [seg1[p - n0] for p in range(max(tb * 16, n0), n)]
    nan_fs = np.zeros((n1, n2), bool)
    for r in rows:
        for c in cols:
            nan_fs[(c, r) if swapped else (r, c)] = True
    assert nan_fs.any() and not nan_fs.all()
    assert np.array_equal(np.isnan(fs), nan_fs) and np.array_equal(np.isnan(sf), nan_fs.T)
    assert_parity(fs[~nan_fs], want_fs[~nan_fs], "written fs")
    assert_parity(sf[~nan_fs.T], want_sf[~nan_fs.T], "written sf")
    rc, fs, sf = j.cross(cfg)                                       # the hook is reset: clean
    assert rc == 0
    assert_parity(fs, want_fs, "fs after the reset")
    assert_parity(sf, want_sf, "sf after the reset")
    j.close()


# ---- 8. other dimensions, the asynchronous form, timing

@pytest.mark.parametrize("dim", [8, 26, 5, 40])
def test_other_dimensions(ctx, oracle, dim):
    """D = 8 and 26: fast kernels; D = 5: zero-padded to 8; D = 40: no fast kernel, the generic one."""
    A, B = ragged(("dims", dim), 21, 37, dim)
    want_fs, want_sf = oracle_cross(oracle, ("dims", dim), A, B, dim, 0.0625)
    for name, mode, bitwise in (("default", "hybrid", dim == 40), ("strict", "strict", True)):
        fs, sf, _ = run_cross(ctx, A, B, dim, 0.0625, UNIT, mode)
        check(fs, want_fs, bitwise, "D = %d %s fs" % (dim, name))
        check(sf, want_sf, bitwise, "D = %d %s sf" % (dim, name))


def test_async_form_and_timing(ctx, oracle, apd):
    n1, n2, dim = 21, 37, 13
    A, B = ragged(("async",), n1, n2, dim)
    cfg = config(0.0625)
    j = Joined(ctx, A, B, dim)
    rc, fs, sf = j.cross(cfg)
    assert rc == 0
    d_fs, d_sf = ctx.alloc(4 * n1 * n2), ctx.alloc(4 * n1 * n2)
    ctx.set_timing(True)
    try:
        apd.check(apd.lib().apd_align_cross_device_async(ctx.handle, j.j.handle, C.byref(cfg), d_fs.at(), d_sf.at()), ctx.handle)
        ctx.synchronize()
        assert ctx.last_kernel_ms() > 0
    finally:
        ctx.set_timing(False)
    assert np.array_equal(d_fs.to_numpy(np.uint32), fs.view(np.uint32).ravel()) and np.array_equal(d_sf.to_numpy(np.uint32), sf.view(np.uint32).ravel())
    d_fs.free()
    d_sf.free()
    j.close()


def test_python_mirror_and_empty_sets(ctx, oracle, apd):
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery
    A, B = ragged(("mirror",), 5, 18, 13)
    want_fs, want_sf = oracle_cross(oracle, ("mirror",), A, B, 13, 0.0625)
    wa, wb = AlignmentWorkers.new([NDSequence(s) for s in A], ctx), AlignmentWorkers.new([NDSequence(s) for s in B], ctx)
    fs, sf = wa.cross(wb, Discovery(warping_band_percentage=0.0625))
    assert_parity(fs, want_fs, "mirror fs")
    assert_parity(sf, want_sf, "mirror sf")
    with pytest.raises(ValueError):
        AlignmentWorkers.cross(type("Multi", (), {"_multi": object()})(), wb, Discovery())
    wa.close()
    wb.close()
    j = Joined(ctx, [], B, 13)                                     # an empty set: APD_OK, nothing written
    rc, fs, sf = j.cross(config(0.0625))
    assert rc == 0 and fs.shape == (0, 18) and apd.lib().apd_batch_first_len(j.j.handle) == 0
    j.close()
