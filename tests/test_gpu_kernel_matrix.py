"""Every instantiated DTW kernel -- (family, geometry, frame dimension) x launch form -- forced through apd_set_variant and compared
with the CPU oracle, with the proof that the NAMED kernel ran.

The matrix is not written here: tests/_kernel_table.py reads the five geometry lists and kKernelDims from csrc/apd_internal.h, so a
geometry added to the header is a new case of this module.  Each case forces one code, aligns a "full" batch (the widest tile
bound 2w + 1 just below the geometry's capacity; for the strips: lengths on either side of a pass boundary G * CW) and a "narrow"
one (idle upper lanes), reads `geometry <code>: <n> tiles` from the APD_DEBUG_PLAN lines, asserts that the forced code took EVERY
tile, and compares the matrix with oracle.align_all.  Every batch spans two tile rows (a diagonal, an off-diagonal and a partly
filled tile), has several distinct lengths (gap widening, directed band) and one exact copy (score 0.0); the full batches hold
sequences of 1, 2 and 3 frames inside sweeping tiles.

Bounds are the suite's own: bitwise equality with the oracle in strict mode (tests/test_gpu_census.py) and wherever the launcher
takes the literal select on strict distances (tests/test_gpu_dtw.py::test_every_systolic_geometry); 1e-4 relative with identical
zeros and +INF pattern everywhere else.  Seeds are fixed.  No case needed the coincidental-tie rule of DESIGN.md section 6 (a
hybrid-mode entry beyond 1e-4 that exact and strict mode do not share): none is re-seeded.

What decides which kernel a tile gets is plan_tile_classes / pick_band_geom / pick_strip_geom (csrc/dtw_generic.hip); the batch
builders below follow those rules and check their own tile bounds with a mirror of the plan's arithmetic (tile_needs).
"""
import collections
import os
import zlib

import numpy as np
import pytest

import _kernel_table as kt

pytestmark = pytest.mark.gpu
RTOL = 1e-4
UNIT, EQUAL, UNEQUAL = (1.0, 1.0, 1.0), (0.7, 0.7, 0.7), (0.6, 1.3, 1.0)

HAVE, DROPPED = kt.pairs()

# family -> [(form, penalties, distance mode, bitwise)].  bitwise = True: the matrix must equal the oracle's bit for bit.
#
# systolic / unit-strict: launch_align (dtw_generic.hip, "part.hybrid = L.hybrid && (... L.dim >= 8 && !L.strict ...)") clears the
#   hybrid form, and launch_systolic (dtw_systolic.h, "if (unit && !L.hybrid) return launch_systolic_strict<D>(L, g, stream);") takes
#   <.., UNIFORM_PEN = true, HYBRID = false> of dtw_sysx.hip: strict distances, and a select that picks the reference's predecessor.
# systolic / unequal: launch_systolic, "if (!unit) launch_systolic_kernel<D, CC, GG, false, false>(L, stream);" -- the literal
#   comparison chain on strict distances.
# banded / unequal and banded / unit-strict: launch_full (dtw_full.h), "const bool general = !((L.band.ins == L.band.del) &&
#   (L.band.del == L.band.mat)) || L.strict;" and "general ? launch_full_general<D, CC, 64 / PP>(L, stream) : ...": GENERAL_PEN, the
#   same literal chain on strict distances, one DP per ordered pair.
# Everything else is a fast distance form (norm expansion, or the fma chain and v_sqrt_f32): 1e-4.  The hybrid form of the wide and
# strip kernels runs from D = 10 with unit penalties only (launch_align: "L.dim >= 10 && L.band.mat == 1.0f"); elsewhere "hybrid"
# and "exact" mode launch the difference form, which is then simply compared twice.
FORMS = {
    "systolic": [("unit-hybrid", UNIT, "hybrid", False), ("unit-exact", UNIT, "exact", False), ("unit-strict", UNIT, "strict", True),
                 ("unequal", UNEQUAL, "hybrid", True)],
    "wide": [("unit-hybrid", UNIT, "hybrid", False), ("unit-exact", UNIT, "exact", False), ("p07-hybrid", EQUAL, "hybrid", False),
             ("p07-exact", EQUAL, "exact", False)],
    "strip": [("unit-hybrid", UNIT, "hybrid", False), ("unit-exact", UNIT, "exact", False), ("p07-hybrid", EQUAL, "hybrid", False),
              ("p07-exact", EQUAL, "exact", False)],
    "banded": [("unit-hybrid", UNIT, "hybrid", False), ("unit-exact", UNIT, "exact", False), ("p07-exact", EQUAL, "exact", False),
               ("unequal", UNEQUAL, "hybrid", True), ("unit-strict", UNIT, "strict", True)],
}

Batch = collections.namedtuple("Batch", "key seqs frames offsets lens pct dup n_tiles")
_batches, _wants = {}, {}


def case_id(fam, a, b, d, form=None):
    return "%s-%d-d%d" % (fam, kt.encode(fam, a, b), d) + ("-" + form if form else "")


def make_batch(key, dim, lens, pct, copy_of):
    """Random-walk sequences of the given lengths in a shuffled caller order, plus an exact copy of the sequence of length
    `copy_of`; cached per key (the oracle's matrices too: _wants)."""
    if key in _batches:
        return _batches[key]
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    lens = [int(v) for v in lens]
    rng.shuffle(lens)
    seqs = [np.cumsum(rng.standard_normal((n, dim)), axis=0).astype(np.float32) * np.float32(0.4) for n in lens]
    src = lens.index(int(copy_of))
    seqs.append(seqs[src].copy())
    lens = lens + [lens[src]]
    assert len(set(lens)) >= 2 and 16 < len(lens) <= 32          # two tile rows: tiles (0, 0), (0, 1) and a partly filled (1, 1)
    offsets = np.zeros(len(seqs) + 1, np.uint64)
    offsets[1:] = np.cumsum(lens)
    _batches[key] = Batch(key, seqs, np.concatenate(seqs, axis=0), offsets, lens, float(pct), (src, len(seqs) - 1), 3)
    return _batches[key]


def tile_needs(lens, pct):
    """2w + 1 per tile with the plan's bound of w (plan_tile_classes: resident order is longest first, 16 sequences per tile row,
    w = max(min(band, longest), longest - shortest) + 2 over the two rows of a tile; the band as host_band_from_pct's f32 product)."""
    order = sorted(lens, reverse=True)
    rows = [order[i:i + 16] for i in range(0, len(order), 16)]
    needs = []
    for x in range(len(rows)):
        for y in range(x, len(rows)):
            mx, mn = max(rows[x][0], rows[y][0]), min(rows[x][-1], rows[y][-1])
            band = int(np.float32(pct) * np.float32(mx))
            needs.append(2 * (max(min(band, mx), mx - mn) + 2) + 1)
    return needs


def uniform_batch(key, dim, length, band):
    """22 sequences of length .. length + 6 under a band of `band` frames: every pair has w = max(band, gap <= 6) + 2."""
    lens = [length + k % 7 for k in range(21)]
    return make_batch(key, dim, lens, (band + 0.5) / (length + 6), length + 3)


def band_form_batch(fam, dim, cap, shape):
    """Systolic and wide kernels.  A forced band-form code takes a tile when its capacity holds the tile's 2w + 1 (pick_band_geom).
    full: M = (cap - 3) // 2 is the longest length whose tiles still fit next to a one-frame sequence (w = M - 1 + 2, 2w + 1 =
    2M + 3 <= cap); the band of the long pairs binds a little (M - 4), so they sweep nearly every offset of the kernel in both
    directions.  narrow: long sweeps under a band that leaves the upper lanes idle."""
    if shape == "full":
        m = (cap - 3) // 2
        if fam == "systolic":
            lens = [max(m - k % 4, 2) for k in range(17)] + [max(m // 2, 3), max(m // 3, 3)]
        else:
            lens = [m, m - 1, m - 2, m - 3] + [m // 2 + 1, m // 2, m // 3, m // 4, 260, 190, 130, 100, 75, 70, 64, 50, 41, 17]
        batch = make_batch((fam, dim, "full", cap), dim, lens + [3, 2, 1, 2, 1, 3], (max(m - 4, 1) + 0.5) / m, m - 1)
        assert cap - 1 <= max(tile_needs(batch.lens, batch.pct)) <= cap
    elif fam == "systolic":
        batch = uniform_batch((fam, dim, "narrow"), dim, 147, 3)
    else:
        lens = [3, 2, 1, 2, 17, 40, 41, 70, 75, 100, 130, 131, 150, 160, 177, 188, 190, 193, 194, 199, 200, 200]
        batch = make_batch((fam, dim, "narrow"), dim, lens, 0.3, 193)
    assert 3 * max(tile_needs(batch.lens, batch.pct)) <= 2 * cap or shape == "full", (batch.key, cap)
    return batch


def strip_batch(dim, wcols, shape):
    """Column strips: a full band (it never binds: plan_tile_classes' first branch), every tile row with a sequence of 3 frames or
    more.  full: lengths on either side of one and two passes of wcols = G * CW columns (columns 1 .. m - 1 are swept).  narrow:
    at most half a pass, the upper lanes of every pair idle."""
    if shape == "full":
        lens = [wcols - 1, wcols, wcols + 1, wcols + 2, 2 * wcols, 2 * wcols + 1, 2 * wcols + 2, wcols + wcols // 2,
                190, 130, 100, 75, 70, 50, 41, 40, 40, 18, 17, 17, 3, 2, 1, 2, 1]
        return make_batch(("strip", dim, "full", wcols), dim, lens, 1.0, wcols + 1)
    h = wcols // 2
    lens = [h + 1, h, h, h - 1, h - 2, h - 3, h - 5, h - 7, max(h // 2, 3), max(h // 2 - 1, 3), max(h // 3, 3), max(h // 4, 3)]
    lens += [min(v, h) for v in (17, 9, 5, 4)] + [3, 2, 1, 2, 1]
    return make_batch(("strip", dim, "narrow", wcols), dim, lens, 1.0, h - 1)


def banded_batch(dim, wcols, shape):
    """Banded column strips: a forced code takes a tile whose rows both hold a sequence of 50 frames or more (cols >= 49) and in
    which the band binds (else equal penalties send the tile down the one-DP branch, which a banded code does not serve).
    full: band 90 % over ragged lengths on either side of one and two passes.  narrow: band 5 % (w follows the length gap) over
    lengths of about half a pass."""
    if shape == "full":
        lens = [wcols - 1, wcols, wcols + 1, wcols + 2, 2 * wcols + 1, 2 * wcols + 2, wcols + wcols // 2, 333, 200, 150, 130, 91, 90,
                90, 75, 61, 60, 55, 50, 3, 2, 1, 2]
        batch = make_batch(("banded", dim, "full", wcols), dim, lens, 0.9, wcols + 1)
    else:
        h = max(wcols // 2, 60)
        lens = [h + 10 - k for k in range(20)] + [50, 3, 2, 1, 2]
        batch = make_batch(("banded", dim, "narrow", wcols), dim, lens, 0.05, h + 8)
    order = sorted(batch.lens, reverse=True)
    assert min(batch.lens) == 1 and order[16] >= 50              # both tile rows: cols >= 49, and the band binds (pct * mx < mx - 3)
    return batch


def batch_for(fam, a, b, dim, shape):
    cap = kt.capacity(fam, a, b)
    if fam in ("systolic", "wide"):
        return band_form_batch(fam, dim, cap, shape)
    if fam == "strip":
        return strip_batch(dim, cap, shape)
    if fam == "banded":
        return banded_batch(dim, cap, shape)
    # shared column rings: the tiles whose workgroups sweep bands of nearly one width (shared_columns_qualify)
    if shape == "full":                                          # every pair w = (cap - 1) // 2: 2w + 1 just below the capacity
        return uniform_batch((fam, dim, "full", cap), dim, max(300, cap + 20), (cap - 1) // 2 - 2)
    if shape == "narrow":
        return uniform_batch((fam, dim, "narrow"), dim, 147, 3)
    lens = [18 + k % 5 for k in range(18)] + [1, 2, 1, 2, 3, 3]      # "tiny": absent result cells inside sweeping workgroups
    return make_batch((fam, dim, "tiny"), dim, lens, 0.5, 20)


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    c.set_distance_mode("hybrid")
    yield c
    c.set_variant(0)
    c.close()


def want_for(oracle, batch, pens):
    key = (batch.key, pens)
    if key not in _wants:
        _wants[key] = oracle.align_all(batch.frames, batch.offsets, batch.pct, *pens, workers=8)
        src, dup = batch.dup
        assert _wants[key][src, dup] == 0.0 and _wants[key][dup, src] == 0.0
    return _wants[key]


def run(ctx, batch, pens, mode, variant, capfd):
    """(matrix, {geometry code: tiles}) of one alignment of `batch` with `variant` forced."""
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery
    n = len(batch.seqs)
    ctx.set_distance_mode(mode)
    ctx.set_variant(variant)
    os.environ["APD_DEBUG_PLAN"] = "1"
    try:
        capfd.readouterr()
        out = AlignmentWorkers.new([NDSequence(s) for s in batch.seqs], ctx).align_all(
            Discovery(warping_band_percentage=batch.pct, insertion_penalty=pens[0], deletion_penalty=pens[1],
                      match_penalty=pens[2])).reshape(n, n).copy()
        plan = kt.read_plan(capfd.readouterr().err)
    finally:
        os.environ.pop("APD_DEBUG_PLAN", None)
        ctx.set_variant(0)
        ctx.set_distance_mode("hybrid")
    return out, plan


def check(got, want, bitwise, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape
    if bitwise:
        differing = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        print("%s: %d of %d entries differ bitwise" % (what, differing, got.size))
        assert differing == 0, "%s: %d of %d entries differ bitwise from the oracle" % (what, differing, got.size)
        return
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got)), what + ": INF/NaN pattern differs"
    assert np.array_equal(np.isposinf(want), np.isposinf(got)), what
    zero = fin & (want == 0)
    assert np.all(got[zero] == 0), what + ": exact zeros (diagonal, identical sequences) must stay 0"
    nz = fin & ~zero
    rel = np.abs(got[nz] - want[nz]) / np.abs(want[nz])
    print("%s: max rel err %.3e over %d entries" % (what, rel.max(), int(nz.sum())))
    assert rel.max() <= RTOL, "%s: max rel err %.3e" % (what, rel.max())


CASES = [(fam, a, b, d, form) for fam, a, b, d in HAVE if fam in FORMS for form in FORMS[fam]]


@pytest.mark.parametrize("fam,a,b,dim,form", CASES, ids=[case_id(f, a, b, d, form[0]) for f, a, b, d, form in CASES])
def test_forced_kernel_takes_every_tile_and_matches_the_oracle(ctx, oracle, capfd, fam, a, b, dim, form):
    name, pens, mode, bitwise = form
    code = kt.encode(fam, a, b)
    for shape in ("full", "narrow"):
        batch = batch_for(fam, a, b, dim, shape)
        got, plan = run(ctx, batch, pens, mode, code, capfd)
        assert plan == {code: batch.n_tiles}, "%s batch of %s: the plan is %r, not every tile on %d" % (shape, case_id(fam, a, b, dim), plan, code)
        check(got, want_for(oracle, batch, pens), bitwise, "%s %s" % (case_id(fam, a, b, dim, name), shape))


SHARED = [p for p in HAVE if p[0] == "shared"]


@pytest.mark.parametrize("fam,a,b,dim", SHARED, ids=[case_id(*p, "unit-hybrid") for p in SHARED])
def test_shared_columns_take_every_tile_and_keep_the_bits_of_their_dpp_twin(ctx, oracle, capfd, fam, a, b, dim):
    """The hybrid form with unit penalties, the only one the plan names the class for (launch_systolic: "if (!(unit && L.hybrid))
    return false;").  Same frames, same arithmetic as the DPP-window kernel G * 100 + C: the same bits."""
    code, twin = kt.encode(fam, a, b), kt.encode("systolic", a, b)
    for shape in ("full", "narrow", "tiny"):
        batch = batch_for(fam, a, b, dim, shape)
        got, plan = run(ctx, batch, UNIT, "hybrid", code, capfd)
        assert plan == {code: batch.n_tiles}, (shape, plan)
        dpp, plan_d = run(ctx, batch, UNIT, "hybrid", twin, capfd)
        assert plan_d == {twin: batch.n_tiles}, (shape, plan_d)
        check(got, want_for(oracle, batch, UNIT), False, "%s %s" % (case_id(fam, a, b, dim, "unit-hybrid"), shape))
        assert np.array_equal(got.view(np.uint32), dpp.view(np.uint32)), "%s: %d entries differ from the DPP twin" % (
            shape, int((got.view(np.uint32) != dpp.view(np.uint32)).sum()))


# ---- documented fallbacks: the forced code names no kernel for these tiles; something else runs and the result is still right

@pytest.mark.parametrize("fam,a,b,dim", DROPPED, ids=[case_id(*p) for p in DROPPED])
def test_a_code_the_dimension_cannot_hold_takes_no_tile(ctx, oracle, capfd, fam, a, b, dim):
    """Every (geometry, D) that max_cells_per_lane / max_strip_columns drop, on a batch that qualifies for the geometry in every
    other respect: geom_instantiated is false, so no tile carries the code.  A mirror that has drifted from the header's clamps
    fails here (it drops a kernel that exists: the code takes tiles) or in the matrix test above (it keeps one that does not)."""
    code = kt.encode(fam, a, b)
    batch = batch_for(fam, a, b, dim, "narrow")
    got, plan = run(ctx, batch, UNIT, "hybrid", code, capfd)
    assert code not in plan and sum(plan.values()) == batch.n_tiles, plan
    check(got, want_for(oracle, batch, UNIT), False, case_id(fam, a, b, dim) + " dropped")


def smallest(fam, dim=13):
    return min((p for p in HAVE if p[0] == fam and p[3] == dim), key=lambda p: kt.capacity(*p[:3]))


@pytest.mark.parametrize("fam", ["systolic", "wide", "shared"])
def test_a_band_wider_than_the_forced_capacity_takes_no_tile(ctx, oracle, capfd, fam):
    """pick_band_geom: "f.capacity() >= need ... ? f : KernelGeom{}" -- every tile of this batch needs more offsets than the
    family's smallest geometry has."""
    _, a, b, dim = smallest(fam)
    cap = kt.capacity(fam, a, b)
    band = cap // 2 + 4
    batch = uniform_batch((fam, dim, "too wide", cap), dim, band + 60, band)
    assert min(tile_needs(batch.lens, batch.pct)) > cap
    code = kt.encode(fam, a, b)
    got, plan = run(ctx, batch, UNIT, "hybrid", code, capfd)
    assert code not in plan and kt.encode("systolic", a, b) not in plan and sum(plan.values()) == batch.n_tiles, plan
    check(got, want_for(oracle, batch, UNIT), False, case_id(fam, a, b, dim) + " too wide")


@pytest.mark.parametrize("fam", ["wide", "strip"])
def test_strict_mode_takes_no_tile_of_a_forced_wide_or_strip_code(ctx, oracle, capfd, fam):
    """Strict mode clears uniform_pen (apd_api.hip: "... && (band.del == band.mat) && !strict"), which is what admits the wide and
    one-DP strip families: other kernels take the tiles, and strict mode stays bit-identical to the oracle."""
    _, a, b, dim = smallest(fam)
    code = kt.encode(fam, a, b)
    batch = batch_for(fam, a, b, dim, "narrow")
    got, plan = run(ctx, batch, UNIT, "strict", code, capfd)
    assert code not in plan and sum(plan.values()) == batch.n_tiles, plan
    check(got, want_for(oracle, batch, UNIT), True, case_id(fam, a, b, dim) + " strict")
