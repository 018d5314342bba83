"""The fast distance forms over the whole f32 feature range: every kernel family compared with the CPU oracle on corpora scaled by
2^k from 2^-80 to 2^59, on mixed magnitudes, one-ulp neighbours, exact zeros, DC offsets and across apd_batch_refill.

The premise is tests/test_oracle.py::test_oracle_is_equivariant_under_power_of_two_scaling: for k in [-60, 55] the scaled corpus
is the same alignment problem one binade over, so nothing in the oracle gives a reason to exempt an entry, and none is.  The
oracle's matrix is computed from the scaled frames at every scale (never by scaling k = 0's), cached per (batch, penalties, k).

The fast kernels serve batches whose features are 0 or have kFeatureFloor = 2^-40 <= |v| < kFeatureBound = 2^60
(csrc/apd_internal.h); pad_frames_kernel flags every other batch, and the literal kernel aligns it.  Every case here asserts
 * the flag (apd_batch_nonfinite) is what the header's two constants say for these frames (kt.leaves_fast_range);
 * unflagged: the forced geometry took every tile (APD_DEBUG_PLAN) and the matrix passes the kernel matrix's own `check` -- same
   finite / INF / NaN pattern, exact zeros stay zero, 1e-4 relative elsewhere, bitwise for the forms that module marks bitwise;
 * flagged: the matrix is the oracle's bit for bit.
Batch builders, `run`, `check` and the oracle cache are those of tests/test_gpu_kernel_matrix.py, imported.

Geometry per family: the smallest-capacity entry of the header's list that exists at the dimension.  The shared column rings have
one geometry, (16, 9), which max_cells_per_lane drops at D = 26: they run at D = 13 and 8, and only in the unit-hybrid form (the
only one the plan names the class for).
"""
import ctypes as C

import numpy as np
import pytest

import _kernel_table as kt
import test_gpu_kernel_matrix as km

pytestmark = pytest.mark.gpu
UNIT, EQUAL, UNEQUAL = km.UNIT, km.EQUAL, km.UNEQUAL
SCALES = [-80, -75, -70, -66, -64, -63, -62, -60, -41, -40, -39, -20, 20, 40, 55, 59]
FLOOR, BOUND = kt.feature_range()


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    c.set_distance_mode("hybrid")
    yield c
    c.set_variant(0)
    c.close()


def form_of(fam, name):
    return next(f for f in km.FORMS[fam] if f[0] == name)


def sweep_cases():
    cases = []
    for fam, dims, names in (("systolic", (13,), ("unit-hybrid", "unit-exact", "unit-strict", "unequal")),
                             ("systolic", (8, 26), ("unit-hybrid", "unit-exact")),
                             ("shared", (13, 8), ("unit-hybrid",)),
                             ("wide", (13,), ("unit-hybrid", "unit-exact", "p07-exact")),
                             ("strip", (13,), ("unit-hybrid", "unit-exact", "p07-exact")),
                             ("banded", (13,), ("unit-hybrid", "unit-exact"))):
        for dim in dims:
            _, a, b, _ = km.smallest(fam, dim)
            for name in names:
                form = ("unit-hybrid", UNIT, "hybrid", False) if fam == "shared" else form_of(fam, name)
                cases.append((fam, a, b, dim, form))
    return cases


SWEEP = sweep_cases()


def scaled(batch, k):
    """`batch` with every feature multiplied by 2^k (exact: ldexp), under a key of its own."""
    if k == 0:
        return batch
    return batch._replace(key=(batch.key, "x 2^k", k), seqs=[np.ldexp(s, k) for s in batch.seqs], frames=np.ldexp(batch.frames, k))


def custom_batch(key, seqs, pct, dup):
    seqs = [np.ascontiguousarray(s, np.float32) for s in seqs]
    offsets = np.zeros(len(seqs) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    assert np.array_equal(seqs[dup[0]], seqs[dup[1]])
    return km.Batch(key, seqs, np.concatenate(seqs, axis=0), offsets, [len(s) for s in seqs], float(pct), dup, (len(seqs) + 15) // 16 * ((len(seqs) + 15) // 16 + 1) // 2)


def flag_of(ctx, apd, frames, offsets, dim):
    """apd_batch_nonfinite of a fresh batch of these frames."""
    from audio_pattern_discovery_amd.alignments import Batch
    b = Batch(ctx, frames, offsets, dim)
    try:
        nf = C.c_int(-1)
        apd.check(apd.lib().apd_batch_nonfinite(ctx.handle, b.handle, C.byref(nf)), ctx.handle)
        return nf.value
    finally:
        b.close()


def run_and_check(ctx, apd, oracle, capfd, batch, pens, mode, code, bitwise, what):
    """One alignment of `batch` under `code` (0: default dispatch) against the oracle; returns (matrix, plan, flag)."""
    got, plan = km.run(ctx, batch, pens, mode, code, capfd)
    want = km.want_for(oracle, batch, pens)
    flag = flag_of(ctx, apd, batch.frames, batch.offsets, batch.frames.shape[1])
    expected = int(kt.leaves_fast_range(batch.frames))
    print("%s: apd_batch_nonfinite %d (the header's range says %d), plan %r" % (what, flag, expected, plan))
    if flag:
        km.check(got, want, True, what + " [flagged: literal kernel]")
    else:
        if code:
            assert plan == {code: batch.n_tiles}, "%s: the plan is %r, not every tile on %d" % (what, plan, code)
        else:
            assert sum(plan.values()) == batch.n_tiles, (what, plan)
        km.check(got, want, bitwise, what)
    assert flag == expected, "%s: apd_batch_nonfinite is %d, the range [2^-40, 2^60) says %d" % (what, flag, expected)
    return got, plan, flag


def expect_flag(batch, k):
    """What the sweep's corpora (random walks x 0.4: |v| from about 1e-5 to about 30) must do at the ends of the range."""
    want = kt.leaves_fast_range(batch.frames)
    if k in (20, 40):
        assert not want, "the 2^%d corpus must stay on the fast kernels" % k
    if k <= -39 or k == 59:
        assert want, "the 2^%d corpus must leave the fast range" % k


@pytest.mark.parametrize("k", SCALES, ids=["2^%d" % k for k in SCALES])
@pytest.mark.parametrize("fam,a,b,dim,form", SWEEP, ids=[km.case_id(f, a, b, d, form[0]) for f, a, b, d, form in SWEEP])
def test_forced_kernel_matches_the_oracle_at_every_scale(ctx, apd, oracle, capfd, fam, a, b, dim, form, k):
    name, pens, mode, bitwise = form
    batch = scaled(km.batch_for(fam, a, b, dim, "full"), k)
    expect_flag(batch, k)
    run_and_check(ctx, apd, oracle, capfd, batch, pens, mode, kt.encode(fam, a, b), bitwise, "%s x 2^%d" % (km.case_id(fam, a, b, dim, name), k))


@pytest.mark.parametrize("k", SCALES, ids=["2^%d" % k for k in SCALES])
@pytest.mark.parametrize("mode", ["hybrid", "exact"])
def test_a_generic_dimension_matches_the_oracle_at_every_scale(ctx, apd, oracle, capfd, mode, k):
    """D = 5 through default dispatch: frames padded to the D = 8 kernels, components 5 .. 7 exact zeros."""
    lens = [60, 59, 58, 57, 40, 33, 30, 30, 24, 20, 17, 12, 9, 8, 5, 4, 3, 2, 1, 2, 1, 3]
    batch = scaled(km.make_batch(("generic", 5, "range"), 5, lens, 0.2, 58), k)
    expect_flag(batch, k)
    run_and_check(ctx, apd, oracle, capfd, batch, UNIT, mode, 0, False, "default dispatch D=5 %s x 2^%d" % (mode, k))


# ---- mixed magnitudes in one batch

def mixed_batches():
    base = kt.mixed_magnitude_corpus()
    rng = np.random.default_rng(11)
    one = rng.standard_normal(base.shape).astype(np.float32)
    one[1] = one[0]
    two = one.copy()
    two[9, 40, 6] = np.float32(1e-25)                               # the ONLY difference from `one`
    return {"tiny-to-huge rows": base, "O(1)": one, "O(1) with one 1e-25": two}


@pytest.mark.parametrize("pct", [0.1, 1.0])
@pytest.mark.parametrize("mode", ["exact", "hybrid"])
@pytest.mark.parametrize("which", ["tiny-to-huge rows", "O(1)", "O(1) with one 1e-25"])
def test_mixed_magnitudes_in_one_batch(ctx, apd, oracle, capfd, which, mode, pct):
    """The corpus of test_strict_distance_bits_with_tiny_zero_and_huge_differences (rows x 1e-30, 3e-20, 2e-15, 1e17, a shift by
    1e-38, identical sequences and frames) in the two fast modes, and an O(1) batch before and after ONE feature becomes 1e-25."""
    base = mixed_batches()[which]
    batch = custom_batch(("mixed", which, pct), list(base), pct, (0, 1))
    assert kt.leaves_fast_range(batch.frames) == (which != "O(1)")
    run_and_check(ctx, apd, oracle, capfd, batch, UNIT, mode, 0, False, "mixed %s, %s, band %g" % (which, mode, pct))


# ---- one-ulp neighbours: squared distances of 2^-124 and below from features that are not small enough for their norms to matter

@pytest.mark.parametrize("mode", ["exact", "hybrid", "strict"])
@pytest.mark.parametrize("e", [-39, -41, -45])
def test_one_ulp_neighbours(ctx, apd, oracle, capfd, e, mode):
    """Features of magnitude [2^e, 2^(e+1)), and copies that differ by +-1 ulp (2^(e-23)) in three components of every frame: the
    squared distance between neighbours is 3 * 2^(2e-46).  e = -39: 2^-124 and up, normal, every feature at or above the floor --
    the fast kernels keep the batch and must be right (frame norms 2^-75: this is not the norms underflowing).  e = -41, -45:
    2^-128, 2^-136, subnormal squares from features far above the exponent at which the norms underflow -- below the floor,
    the literal kernel's.  Strict mode rides along (bitwise): its square root leaves the v_sqrt_f32 fix-up below 2^-96."""
    rng = np.random.default_rng(1000 - e)
    lens = [40, 40, 39, 37, 33, 30, 26, 21, 12, 5]
    seqs = []
    for n in lens:
        mant = (1.0 + rng.random((n, 13))) * rng.choice([-1.0, 1.0], size=(n, 13))
        seqs.append(np.ldexp(mant, e).astype(np.float32))
    for s in list(seqs):
        bits = s.view(np.uint32).copy()
        for t in range(len(s)):
            comps = rng.choice(13, size=3, replace=False)
            step = rng.choice([-1, 1], size=3)
            mant = (bits[t, comps] & 0x7FFFFF).astype(np.int64)     # stay inside the binade: a step that would leave it is reversed
            step = np.where((mant + step < 0) | (mant + step > 0x7FFFFF), -step, step)
            bits[t, comps] = (bits[t, comps].astype(np.int64) + step).astype(np.uint32)
        seqs.append(bits.view(np.float32))
    seqs.append(seqs[0].copy())
    mags = np.abs(np.concatenate(seqs))
    assert mags.min() >= 2.0 ** e and mags.max() < 2.0 ** (e + 1)
    batch = custom_batch(("ulp", e), seqs, 0.25, (0, len(seqs) - 1))
    want = km.want_for(oracle, batch, UNIT)
    assert 0 < want[0, 10] <= 2.0 ** (e - 21) and kt.leaves_fast_range(batch.frames) == (e < -40)
    run_and_check(ctx, apd, oracle, capfd, batch, UNIT, mode, 0, mode == "strict", "one-ulp neighbours at 2^%d, %s" % (e, mode))


# ---- exact zeros are inside the range

@pytest.mark.parametrize("fam,mode", [("systolic", "hybrid"), ("systolic", "exact"), ("shared", "hybrid"), ("wide", "hybrid"), ("wide", "exact"),
                                      ("strip", "hybrid"), ("strip", "exact")])
def test_exact_zeros_stay_on_the_fast_kernels(ctx, apd, oracle, capfd, fam, mode):
    """Silence padding (all-zero frames at both ends), whole all-zero sequences and zero components beside O(1) ones: not small
    features.  The batch is unflagged and the forced fast geometry takes every tile."""
    _, a, b, dim = km.smallest(fam)
    src = km.batch_for(fam, a, b, dim, "full")
    seqs = [s.copy() for s in src.seqs]
    dup_src, dup = src.dup
    for i, s in enumerate(seqs):
        if i % 3 == 0:
            s[:len(s) // 4] = 0                                     # leading silence
        if i % 4 == 1:
            s[len(s) - len(s) // 5:] = 0                            # trailing silence
        s[:, (i % 13)] = 0                                          # one dead channel per sequence
        s[::7, 3] = 0
    whole = [i for i in range(len(seqs)) if i not in (dup_src, dup) and len(seqs[i]) > 3][:2]
    for i in whole:
        seqs[i][:] = 0                                              # two all-zero sequences: they score 0.0 against each other
    seqs[dup] = seqs[dup_src].copy()
    batch = src._replace(key=(src.key, "zeros"), seqs=seqs, frames=np.concatenate(seqs, axis=0))
    assert not kt.leaves_fast_range(batch.frames) and (batch.frames == 0).mean() > 0.1
    want = km.want_for(oracle, batch, UNIT)
    assert want[whole[0], whole[1]] == 0.0
    code = kt.encode(fam, a, b)
    got, plan, flag = run_and_check(ctx, apd, oracle, capfd, batch, UNIT, mode, code, False, "zeros %s %s" % (km.case_id(fam, a, b, dim), mode))
    assert flag == 0 and plan == {code: batch.n_tiles}


# ---- DC offset: every cell of the hybrid form in its cancellation recompute

@pytest.mark.parametrize("share", ["all", "half"])
@pytest.mark.parametrize("offset", [1e2, 1e4, 1e6, 3e7])
@pytest.mark.parametrize("fam", ["systolic", "shared", "wide"])
def test_dc_offset_hybrid(ctx, apd, oracle, capfd, fam, offset, share):
    """offset + walk, rounded to f32.  With the offset on every sequence |x|^2 + |y|^2 is 1e4 .. 1e15 times the squared distance:
    every cell falls below tau * (|x|^2 + |y|^2) and takes the difference-form recompute.  On half of them: both regimes in one
    tile.  At 3e7 the ulp is 2: the walk quantises to even integers, identical frames and structural ties appear."""
    _, a, b, dim = km.smallest(fam)
    src = km.batch_for(fam, a, b, dim, "full")
    dup_src, dup = src.dup
    seqs = []
    for i, s in enumerate(src.seqs):
        on = share == "all" or (i if i != dup else dup_src) % 2 == 0
        seqs.append((s + np.float32(offset)).astype(np.float32) if on else s.copy())
    batch = src._replace(key=(src.key, "dc", offset, share), seqs=seqs, frames=np.concatenate(seqs, axis=0))
    assert not kt.leaves_fast_range(batch.frames)
    code = kt.encode(fam, a, b)
    run_and_check(ctx, apd, oracle, capfd, batch, UNIT, "hybrid", code, False, "dc %g on %s, %s" % (offset, share, km.case_id(fam, a, b, dim)))


# ---- refill: the flag and its host copy follow the new values

def test_refill_moves_a_resident_batch_out_of_the_fast_range_and_back(ctx, apd, oracle):
    from audio_pattern_discovery_amd.alignments import Batch
    from audio_pattern_discovery_amd.discovery import Discovery
    _, a, b, dim = km.smallest("systolic")
    src = km.batch_for("systolic", a, b, dim, "full")
    tiny = scaled(src, -70)
    n = len(src.seqs)
    cfg = Discovery(warping_band_percentage=src.pct).align_config()
    L = apd.lib()

    def flag(bt):
        nf = C.c_int(-1)
        apd.check(L.apd_batch_nonfinite(ctx.handle, bt.handle, C.byref(nf)), ctx.handle)
        return nf.value

    def align(bt):
        out = np.empty((n, n), np.float32)
        apd.check(L.apd_align_all(ctx.handle, bt.handle, C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_float))), ctx.handle)
        return out

    def refill(bt, frames):
        frames = np.ascontiguousarray(frames, np.float32)
        apd.check(L.apd_batch_refill(ctx.handle, bt.handle, C.c_void_p(frames.ctypes.data), 0), ctx.handle)

    ctx.set_distance_mode("hybrid")
    ctx.set_variant(0)
    resident = Batch(ctx, src.frames, src.offsets, dim)
    try:
        assert flag(resident) == 0                                  # read back: the host now holds a copy of the flag
        first = align(resident)
        km.check(first, km.want_for(oracle, src, UNIT), False, "refill: O(1)")
        refill(resident, tiny.frames)
        got = align(resident)                                       # aligned BEFORE the flag is asked for: the device-side choice
        km.check(got, km.want_for(oracle, tiny, UNIT), True, "refill: x 2^-70")
        assert flag(resident) == 1
        km.check(align(resident), km.want_for(oracle, tiny, UNIT), True, "refill: x 2^-70, flag known to the host")
        refill(resident, src.frames)
        assert flag(resident) == 0
        back = align(resident)
        km.check(back, km.want_for(oracle, src, UNIT), False, "refill: back to O(1)")
        assert np.array_equal(back.view(np.uint32), first.view(np.uint32))
    finally:
        resident.close()
