"""The hybrid form's cancellation gate -- "recompute the cell in the difference form where |x|^2 + |y|^2 - 2 x.y falls below
tau (|x|^2 + |y|^2)" -- driven through apd_set_distance_mode's tau in every kernel body that has it: dtw_fused_systolic<.., HYBRID>,
dtw_fused_systolic_shared (csrc/dtw_systolic.h), the wide kernel (csrc/dtw_wide.h) and dtw_full_matrix<.., HYBRID, BANDED = false /
true> (csrc/dtw_full.h: strips and banded strips).

At the default tau = 1/64 random walks enter the recompute only around their one duplicated pair.  Here
 1. the knob's contract: NaN and negative values refused, 0 and -0.0 keep the value, the value is sticky across mode changes and
    private to a context, exact and strict mode ignore it -- and a control that shows tau REACHES each family's kernel;
 2. tau = 4: d^2 <= 2 (|x|^2 + |y|^2), so every cell with a non-zero norm sum passes the per-cell test -- every cell of every
    instantiation (family, geometry, D) is the recomputed one;
 3. tau = tau_mid(batch), the median of d^2 / (|x|^2 + |y|^2) over the batch's cross-sequence frame pairs: about every other cell is
    recomputed, hits and misses side by side inside one macro-step, in every instantiation;
 4. one batch, every geometry that can take it, at the default tau, tau_mid and 4: the hybrid per-cell arithmetic is the same in all
    five bodies (frame_sq_expanded_pre, frame_sq_exact_pre, v_sqrt_f32, a per-cell test that does not depend on the wave-level
    one), so every forced matrix has the bits of the default-dispatch matrix.
What the inputs are claimed to do (the share of cells below each threshold) is checked without a GPU in
tests/test_tau_gate_inputs.py.  Batches, `run`, `want_for`, `check` and `case_id` are those of tests/test_gpu_kernel_matrix.py,
imported; the bound is the suite's 1e-4 with identical zeros and +INF pattern.  tau is sticky and km.run resets the mode with
tau = 0 (keep): this module has a context of its own, and every case restores kt.default_tau() in a `finally`.
"""
import contextlib
import zlib

import numpy as np
import pytest

import _kernel_table as kt
import test_gpu_kernel_matrix as km

pytestmark = pytest.mark.gpu
UNIT = km.UNIT
TAU_ALL = 4.0                      # above d^2 / (|x|^2 + |y|^2) <= 2 for every frame pair
TAU_NONE = 2.0 ** -30              # the plumbing control: below the ratio of every cell of the DC-offset batches but the copies'
SAMPLE = 20000
CROSS_DIMS = (10, 13, 16, 20, 26)

LIVE = [p for p in km.HAVE if kt.hybrid_live(p[0], p[3])]


def shapes_of(fam):
    return ("full", "narrow", "tiny") if fam == "shared" else ("full", "narrow")


# ---- the inputs: how many cells a threshold sends through the recompute

_ratios = {}


def gate_ratios(batch):
    """d^2 / (|x|^2 + |y|^2) in float64 of a fixed-seed sample of SAMPLE frame pairs from two different sequences of the batch;
    pairs with a zero norm sum are left out."""
    if batch.key not in _ratios:
        rng = np.random.default_rng(zlib.crc32(repr(("gate sample", batch.key)).encode()))
        frames = batch.frames.astype(np.float64)
        owner = np.repeat(np.arange(len(batch.lens)), batch.lens)
        i = rng.integers(0, len(frames), 3 * SAMPLE)
        j = rng.integers(0, len(frames), 3 * SAMPLE)
        keep = owner[i] != owner[j]
        x, y = frames[i[keep]], frames[j[keep]]
        norms = (x * x).sum(axis=1) + (y * y).sum(axis=1)
        ratio = (((x - y) ** 2).sum(axis=1))[norms > 0] / norms[norms > 0]
        assert len(ratio) >= SAMPLE, (batch.key, len(ratio))
        _ratios[batch.key] = ratio[:SAMPLE]
    return _ratios[batch.key]


def tau_mid(batch):
    """The threshold that about every other cell of `batch` falls below: the median of gate_ratios, as the f32 the library takes."""
    return float(np.float32(np.median(gate_ratios(batch))))


def hit_share(batch, tau):
    return float((gate_ratios(batch) < tau).mean())


# ---- one batch for several families (step 4)

def shared_slack(g, c):
    """shared_column_slack (csrc/apd_internal.h): the spread of w one workgroup of the shared column rings tolerates."""
    unroll = c + 1 if (c + 1) % 2 == 0 else 2 * (c + 1)
    ring_min = (g - 1) * (c - 1) + 1 + 2 * unroll
    return (ring_min + 16 + 7) // 8 * 8 - ring_min


def cross_batch(dim):
    """Full band, lengths <= 68 with 1, 2 and 3 frames among them: 2w + 1 <= 2 (68 + 2) + 1 = 141 in every tile, the shape
    tests/test_gpu_cross.py spans the families with.  Every tile row has a sequence of 3 frames or more (the strips); the band
    never binds (plan_tile_classes' first branch); with a full band w = longer length + 2, and any four neighbours of the
    resident (longest first) order lie within the shared rings' slack (shared_columns_qualify, sequences of one frame aside)."""
    lens = [68, 67, 65, 64, 60, 58, 55, 52, 48, 45, 43, 40, 36, 33, 30, 27, 24, 21, 18, 15, 12, 9, 6, 3, 2, 1, 1]
    batch = km.make_batch(("tau cross", dim), dim, lens, 1.0, 43)
    order = sorted((v for v in batch.lens if v >= 2), reverse=True)
    geoms, _ = kt.parse_table()
    slack = min(shared_slack(g, c) for g, c in geoms["shared"])
    assert all(order[k] - order[min(k + 3, len(order) - 1)] <= slack for k in range(len(order)))   # any four neighbours
    assert max(km.tile_needs(batch.lens, batch.pct)) == 141 and sorted(batch.lens, reverse=True)[16] >= 3
    return batch


def cross_banded_batch(dim):
    """The band binds (5 %: w follows the length gap, up to 70 - 1 + 2) and both tile rows hold a sequence of 50 frames or more: the
    tiles a forced banded-strip code takes (km.banded_batch), still within 2w + 1 <= 143 for the systolic and wide geometries."""
    lens = [70 - k for k in range(20)] + [50, 3, 2, 1, 2]
    batch = km.make_batch(("tau cross banded", dim), dim, lens, 0.05, 62)
    order = sorted(batch.lens, reverse=True)
    assert order[16] >= 50 and int(np.float32(batch.pct) * np.float32(order[0])) < order[0] - 3
    assert max(km.tile_needs(batch.lens, batch.pct)) == 143
    return batch


def takers(batch, dim, families):
    """[(family, a, b)] of `families` whose hybrid kernel exists at dim and takes every tile of `batch` when forced: the band forms
    by capacity (pick_band_geom: "f.capacity() >= need"), the strips whatever the lengths (they sweep in passes)."""
    need = max(km.tile_needs(batch.lens, batch.pct))
    return [(fam, a, b) for fam, a, b, d in LIVE
            if d == dim and fam in families and (fam in ("strip", "banded") or kt.capacity(fam, a, b) >= need)]


CROSS_FAMILIES = ("systolic", "shared", "wide", "strip")
BANDED_FAMILIES = ("banded", "systolic", "wide")


def tau_of(name, batch):
    return {"default": kt.default_tau(), "mid": tau_mid(batch), "all": TAU_ALL}[name]


# ---- running

@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    c.set_distance_mode("hybrid", kt.default_tau())
    yield c
    c.set_variant(0)
    c.close()


@contextlib.contextmanager
def tau_set(ctx, tau):
    """Hybrid mode at `tau` for the body; the default value and hybrid mode afterwards, whatever the body did."""
    ctx.set_distance_mode("hybrid", tau)
    try:
        yield
    finally:
        ctx.set_distance_mode("hybrid", kt.default_tau())


def align(ctx, batch):
    """One alignment of `batch` in whatever mode, tau and variant `ctx` holds."""
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery
    n = len(batch.seqs)
    return AlignmentWorkers.new([NDSequence(s) for s in batch.seqs], ctx).align_all(
        Discovery(warping_band_percentage=batch.pct, insertion_penalty=1.0, deletion_penalty=1.0, match_penalty=1.0)).reshape(n, n).copy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def dc_batch(src, offset=1e4):
    """tests/test_gpu_feature_range.py::test_dc_offset_hybrid's batch, offset on every sequence (same key: one oracle matrix)."""
    seqs = [(s + np.float32(offset)).astype(np.float32) for s in src.seqs]
    return src._replace(key=(src.key, "dc", offset, "all"), seqs=seqs, frames=np.concatenate(seqs, axis=0))


def knob_batch():
    """20 short sequences riding on 1e4: |x|^2 + |y|^2 is about 2.6e9 (ulp 256) over squared distances below 200, so the norm
    expansion has no digit of them, the default tau recomputes every cell, and tau = 2^-30 (threshold about 2.4) recomputes only the
    cells whose expansion came out at or below 0 -- the two matrices differ, which is what makes tau observable below."""
    return dc_batch(km.make_batch(("tau knob", 13), 13, [24 - k % 6 for k in range(17)] + [3, 2, 1], 0.5, 22))


@pytest.fixture(scope="module")
def knob(ctx, oracle):
    """(batch, matrix at the default tau, matrix at tau = 2^-30) through default dispatch."""
    batch = knob_batch()
    assert hit_share(batch, kt.default_tau()) == 1.0 and hit_share(batch, TAU_NONE) < 0.01
    ctx.set_variant(0)
    with tau_set(ctx, kt.default_tau()):
        m_def = align(ctx, batch)
    with tau_set(ctx, TAU_NONE):
        m_low = align(ctx, batch)
    km.check(m_def, km.want_for(oracle, batch, UNIT), False, "tau knob batch, default tau")
    assert not same_bits(m_def, m_low), "tau = 2^-30 gives the default tau's matrix: the batch does not show the knob"
    return batch, m_def, m_low


# ---- 1. the knob's contract

@pytest.mark.parametrize("bad", [float("nan"), -1.0, -2.0 ** -140, float("-inf")], ids=["nan", "-1", "-denormal", "-inf"])
def test_a_nan_or_negative_tau_is_refused_and_changes_nothing(ctx, apd, knob, bad):
    batch, m_def, m_low = knob
    with tau_set(ctx, TAU_NONE):
        for mode in (0, 1, 2):                                   # a refused call sets neither the mode nor the value
            assert apd.lib().apd_set_distance_mode(ctx.handle, mode, bad) == apd.APD_ERR_INVALID_ARG
        assert same_bits(align(ctx, batch), m_low)
    assert same_bits(align(ctx, batch), m_def)


@pytest.mark.parametrize("keep", [0.0, -0.0], ids=["0", "-0"])
def test_tau_zero_keeps_the_current_value(ctx, apd, knob, keep):
    batch, m_def, m_low = knob
    with tau_set(ctx, TAU_NONE):
        assert apd.lib().apd_set_distance_mode(ctx.handle, 1, keep) == apd.APD_OK
        assert same_bits(align(ctx, batch), m_low)
        ctx.set_distance_mode("hybrid")                          # the Python default is tau = 0
        assert same_bits(align(ctx, batch), m_low)
    assert apd.lib().apd_set_distance_mode(ctx.handle, 1, keep) == apd.APD_OK
    assert same_bits(align(ctx, batch), m_def)


def test_a_set_tau_survives_a_round_through_the_other_modes(ctx, oracle, knob):
    batch, m_def, m_low = knob
    want = km.want_for(oracle, batch, UNIT)
    with tau_set(ctx, TAU_NONE):
        ctx.set_distance_mode("strict")
        km.check(align(ctx, batch), want, True, "tau knob batch, strict")
        ctx.set_distance_mode("exact")
        km.check(align(ctx, batch), want, False, "tau knob batch, exact")
        ctx.set_distance_mode("hybrid")
        assert same_bits(align(ctx, batch), m_low)
    assert same_bits(align(ctx, batch), m_def)


@pytest.mark.parametrize("mode", ["exact", "strict"])
def test_exact_and_strict_mode_ignore_tau(ctx, knob, mode):
    batch = knob[0]
    try:
        ctx.set_distance_mode(mode, kt.default_tau())
        at_default = align(ctx, batch)
        ctx.set_distance_mode(mode, TAU_ALL)
        at_four = align(ctx, batch)
        ctx.set_distance_mode(mode, TAU_NONE)
        at_none = align(ctx, batch)
    finally:
        ctx.set_distance_mode("hybrid", kt.default_tau())
    assert same_bits(at_default, at_four) and same_bits(at_default, at_none)


def test_two_contexts_hold_their_own_tau(ctx, apd, knob):
    batch, m_def, m_low = knob
    other = apd.Context(0)
    try:
        other.set_distance_mode("hybrid", TAU_NONE)
        assert same_bits(align(ctx, batch), m_def)               # untouched by the other context's value
        assert same_bits(align(other, batch), m_low)
        with tau_set(ctx, TAU_NONE):
            other.set_distance_mode("hybrid", kt.default_tau())
            assert same_bits(align(ctx, batch), m_low)
            assert same_bits(align(other, batch), m_def)
        assert same_bits(align(other, batch), m_def)
    finally:
        other.close()


@pytest.mark.parametrize("fam", list(kt.FAMILIES))
def test_tau_reaches_the_kernel_of_every_family(ctx, oracle, capfd, fam):
    """Without this a kernel that ignored tau would pass everything below: on the DC-offset batch a gate at 2^-30 leaves the
    expansion's cancelled values in place (the matrix differs from the default tau's), and a gate at 4 is right to 1e-4."""
    _, a, b, dim = km.smallest(fam)
    assert kt.hybrid_live(fam, dim)
    batch = dc_batch(km.batch_for(fam, a, b, dim, "full"))
    assert hit_share(batch, TAU_NONE) < 0.01 and hit_share(batch, kt.default_tau()) == 1.0
    code = kt.encode(fam, a, b)
    got = {}
    for name, tau in (("default", kt.default_tau()), ("2^-30", TAU_NONE), ("4", TAU_ALL)):
        with tau_set(ctx, tau):
            got[name], plan = km.run(ctx, batch, UNIT, "hybrid", code, capfd)
        assert plan == {code: batch.n_tiles}, (name, plan)
    differing = int((got["default"].view(np.uint32) != got["2^-30"].view(np.uint32)).sum())
    print("%s: %d of %d entries differ between tau = 1/64 and tau = 2^-30" % (km.case_id(fam, a, b, dim), differing, got["default"].size))
    assert differing >= 1, "tau does not reach %s" % km.case_id(fam, a, b, dim)
    km.check(got["4"], km.want_for(oracle, batch, UNIT), False, "dc 1e4, tau 4, %s" % km.case_id(fam, a, b, dim))


# ---- 2. and 3.: every cell recomputed / hits and misses interleaved, in every instantiation

def gate_case(ctx, oracle, capfd, fam, a, b, dim, tau_name):
    code = kt.encode(fam, a, b)
    for shape in shapes_of(fam):
        batch = km.batch_for(fam, a, b, dim, shape)
        tau = tau_of(tau_name, batch)
        with tau_set(ctx, tau):
            got, plan = km.run(ctx, batch, UNIT, "hybrid", code, capfd)
        assert plan == {code: batch.n_tiles}, "%s batch of %s: the plan is %r, not every tile on %d" % (shape, km.case_id(fam, a, b, dim), plan, code)
        want = km.want_for(oracle, batch, UNIT)
        km.check(got, want, False, "%s %s tau-%s (%.4g)" % (km.case_id(fam, a, b, dim), shape, tau_name, tau))
        src, dup = batch.dup
        assert got[src, dup] == 0.0 and got[dup, src] == 0.0 and not np.any(np.diag(got))
        assert np.array_equal(np.isposinf(got), np.isposinf(want))


@pytest.mark.parametrize("fam,a,b,dim", LIVE, ids=[km.case_id(*p, "tau-all") for p in LIVE])
def test_every_cell_recomputed_matches_the_oracle(ctx, oracle, capfd, fam, a, b, dim):
    gate_case(ctx, oracle, capfd, fam, a, b, dim, "all")


@pytest.mark.parametrize("fam,a,b,dim", LIVE, ids=[km.case_id(*p, "tau-mid") for p in LIVE])
def test_hits_and_misses_interleaved_match_the_oracle(ctx, oracle, capfd, fam, a, b, dim):
    gate_case(ctx, oracle, capfd, fam, a, b, dim, "mid")


# ---- 4. one answer across kernels

def one_answer(ctx, oracle, capfd, batch, dim, families, tau_name):
    tau = tau_of(tau_name, batch)
    geoms = takers(batch, dim, families)
    exist = {p[0] for p in LIVE if p[3] == dim and p[0] in families}     # (the shared rings' one geometry is dropped from D = 16)
    assert {g[0] for g in geoms} == exist, "no geometry of %r takes the batch at D = %d" % (exist - {g[0] for g in geoms}, dim)
    with tau_set(ctx, tau):
        ref, plan = km.run(ctx, batch, UNIT, "hybrid", 0, capfd)
        assert sum(plan.values()) == batch.n_tiles, plan
        km.check(ref, km.want_for(oracle, batch, UNIT), False, "%s default dispatch %r tau-%s" % (batch.key, plan, tau_name))
        differ = {}
        for fam, a, b in geoms:
            code = kt.encode(fam, a, b)
            got, plan = km.run(ctx, batch, UNIT, "hybrid", code, capfd)
            assert plan == {code: batch.n_tiles}, "%s: the plan is %r, not every tile on %d" % (km.case_id(fam, a, b, dim), plan, code)
            n = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
            if n:
                differ[km.case_id(fam, a, b, dim)] = n
    print("%s tau-%s (%.4g): %d geometries, %d differ from default dispatch: %r" % (batch.key, tau_name, tau, len(geoms), len(differ), differ))
    assert not differ, "entries that differ bitwise from the default-dispatch matrix, per forced geometry: %r" % differ


@pytest.mark.parametrize("tau_name", ["default", "mid", "all"])
@pytest.mark.parametrize("dim", CROSS_DIMS)
def test_every_kernel_that_takes_a_tile_gives_the_same_bits(ctx, oracle, capfd, dim, tau_name):
    one_answer(ctx, oracle, capfd, cross_batch(dim), dim, CROSS_FAMILIES, tau_name)


@pytest.mark.parametrize("tau_name", ["default", "mid", "all"])
@pytest.mark.parametrize("dim", CROSS_DIMS)
def test_banded_strips_give_the_bits_of_the_band_kernels(ctx, oracle, capfd, dim, tau_name):
    one_answer(ctx, oracle, capfd, cross_banded_batch(dim), dim, BANDED_FAMILIES, tau_name)
