"""Every instantiated spotting kernel -- spot_kernel<Kind, RT, D> of csrc/dtw_spot_sweep.h for the kinds SpotSweep ("sweep",
csrc/dtw_spot.hip) and SpotRecordSweep ("record", csrc/dtw_spot_path.hip), both spot_sweep<RT, D, REC> of that header -- against the
checkers, with the proof that the NAMED kernel ran.

The matrix is not written here: tests/_kernel_table.py reads kKernelDims and kSpotRegisterRows from csrc/apd_internal.h, and
tests/_spot_matrix.py builds one case per <RT, D> from them, so a dimension or a register-row class added to the header is a new
case of this module.  Every call runs under APD_DEBUG_PLAN and asserts, from the kernels' own lines, that exactly the intended
instantiation took exactly the intended number of pairs and that no other spotting kernel was launched; the last test asserts
that the lines seen over the module name every instantiation of both kinds.

Per register class R the query lengths include 64 (R - 1) + 1 and 64 R and put query row n on every row of its lane; the LDS class
runs kSpotRegisterRows + 1 and + 2 rows per lane; the two streams are shorter and longer than a wavefront and make m + lane_n even
and odd (the sweep takes two macro-steps per turn).  Unit penalties everywhere, (1, 2, 0.5) for one length per class.  The kernels
with rows in registers get three more pairs that send macro-steps down both square-root branches: planted copies of query frames
(d2 = 0 in otherwise Gaussian data), a pair scaled by 2^-50 (d2 on both sides of 2^-96) and one scaled by 2^62 (d2 on both sides
of overflow); that these pairs do what they are for is asserted on the CPU first.  Dimensions above the largest kernel dimension
run <0, 0>: four consecutive ones (the squared-norm slot of the resident frame in each float4 component) and one further up,
each with a pair of small integers.

Every comparison is bitwise, with the canaries and helpers of tests/test_gpu_spot.py (cost, start, best against
tests/_spot_reference.py) and tests/test_gpu_spot_paths.py (steps, found start, score against tests/_spot_path_reference.py)."""
import numpy as np
import pytest

import _kernel_table as kt
import _spot_matrix as sm
import _spot_path_reference as path_ref
from test_gpu_spot import assert_same, make_batch, raw_spot, reference
from test_gpu_spot_paths import assert_window, raw_curves, raw_paths

pytestmark = pytest.mark.gpu
UNIT, SKEWED = sm.UNIT, sm.SKEWED

REGISTER_KERNELS = sm.register_kernels()
ANY_DIMENSIONS = sm.any_dimensions(kt.parse_dims(kt.header_text()))
_seen = set()                                   # (kind, RT, D) of every spotting-kernel line read in this module


def kernel_id(kernel):
    return "<%d, %d>" % kernel


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    yield c
    c.close()


def assert_dispatch(err, kind, case, pairs):
    """Exactly case.kernel of `kind` took exactly the distinct pairs of `pairs`; for the LDS class, sized for the longest query."""
    rt, d = case.kernel
    launches = kt.read_spot_launches(err)
    plan = kt.read_spot_plan(err)
    _seen.update(plan)
    assert plan == {(kind, rt, d): len(set(pairs))}, "%s of %s: the spotting kernels that ran are %r" % (kind, kernel_id(case.kernel), plan)
    assert len(launches) == 1
    if rt == 0:
        r_max = max(kt.spot_rows_per_lane(case.lengths[x]) for x, _ in pairs)
        assert (launches[0]["r_max"], launches[0]["lds"]) == (r_max, r_max * 64 * 8), launches
    else:
        assert launches[0]["r_max"] is None and launches[0]["lds"] is None


def assert_case_inputs(case, register_rows):
    """What the case is for, shown on the CPU: the row classes, query row n on every row of its lane, both parities of m + lane_n,
    and for the gate pairs cells (and, for the plants, whole macro-steps) on both sides of the square-root gate."""
    rt, d = case.kernel
    queries = sorted({case.lengths[x] for x, _ in case.unit_pairs})
    if d > 0:
        pairs = case.unit_pairs + case.skewed_pairs + case.gate_pairs + case.tie_pairs
        assert {kt.spot_row_class(kt.kernel_dim(case.dim), case.lengths[x]) for x, _ in pairs} == {rt}
        assert kt.kernel_dim(case.dim) == d == case.dim
    else:
        assert kt.kernel_dim(case.dim) == case.dim and kt.spot_row_class(case.dim, 1) == 0      # no kernel dimension: <0, 0> whatever R
    if rt > 0:
        assert queries[0] == 64 * (rt - 1) + 1 and queries[-1] == 64 * rt
        assert {kt.spot_row_n(n)[1] for n in queries} == set(range(rt)), queries
        assert len(case.gate_pairs) == 3
    elif d > 0:
        assert [kt.spot_rows_per_lane(n) for n in queries] == [register_rows + 1, register_rows + 2]
    assert {(case.lengths[y] + kt.spot_row_n(case.lengths[x])[0]) % 2 for x, y in case.unit_pairs} == {0, 1}
    assert min(case.lengths[y] for _, y in case.unit_pairs) < 64 < max(case.lengths[y] for _, y in case.unit_pairs)
    for k, (x, y) in enumerate(case.gate_pairs):
        inside, outside = sm.gate_sides(case.seqs[x], case.seqs[y])
        steps = sm.macro_step_in_domain(case.seqs[x], case.seqs[y], rt)
        print("%s gate pair %d: %d cells in domain, %d outside; %d macro-steps in domain, %d not" % (
            kernel_id(case.kernel), k, inside, outside, int(steps.sum()), int((~steps).sum())))
        assert inside > 0 and outside > 0
        assert steps.any() and not steps.all()                  # whole macro-steps on either side of the wave-wide gate
        if k == 0:
            xs, ys = case.seqs[x], case.seqs[y]
            planted = {c for c in range(len(ys)) if (xs == ys[c]).all(axis=1).any()}
            assert len(planted) == 3 and not planted & {0, len(ys) - 1} and not (xs[-1] == ys).all(axis=1).any()


def sweep_case(apd, ctx, capfd, case, register_rows):
    assert_case_inputs(case, register_rows)
    key = ("matrix", case.kernel, case.dim)
    batch = make_batch(ctx, case.seqs)
    try:
        unit = case.unit_pairs + case.gate_pairs + case.tie_pairs
        for pen, pairs in ((UNIT, unit), (SKEWED, case.skewed_pairs)):
            with kt.debug_plan(capfd) as err:
                got, best, _ = raw_spot(apd, ctx, batch, pen, pairs)
            assert_dispatch(err[0], "sweep", case, pairs)
            for p, (x, y) in enumerate(pairs):
                assert_same(got[p], best[p], reference(key, case.seqs, pen, x, y), "%s %s pair (%d, %d)" % (kernel_id(case.kernel), pen, x, y))
            if pen == UNIT:
                with kt.debug_plan(capfd) as err:
                    none, alone, _ = raw_spot(apd, ctx, batch, pen, pairs, curves=False)
                assert_dispatch(err[0], "sweep", case, pairs)
                assert none == [] and np.array_equal(alone.view(np.uint32), best.view(np.uint32))
    finally:
        batch.close()


def record_case(apd, ctx, capfd, case):
    key = ("matrix", case.kernel, case.dim)
    batch = make_batch(ctx, case.seqs)
    try:
        unit = case.unit_pairs + case.gate_pairs + case.tie_pairs
        for pen, pairs, ends_of in ((UNIT, unit, sm.ends_of), (SKEWED, case.skewed_pairs, sm.ends_of),
                                    (UNIT, [p for p in case.unit_pairs if case.lengths[p[1]] > 64], lambda m: sm.long_ends(m)[:3])):
            curves = raw_curves(apd, ctx, batch, pen, pairs)
            records = [(x, y, end, int(start[end - 1])) for (x, y), (_, start) in zip(pairs, curves) for end in ends_of(case.lengths[y])]
            costs = [cost[end - 1:end] for (x, y), (cost, _) in zip(pairs, curves) for end in ends_of(case.lengths[y])]
            swept = [(x, y) for x, y, _, start in records if start >= 1]             # a window without a start owns no slots: no sweep
            if ends_of is not sm.ends_of:
                assert all(max(r[2] for r in records if r[:2] == p) < case.lengths[p[1]] for p in pairs)   # max_end below m
            with kt.debug_plan(capfd) as err:
                paths, found, scores = raw_paths(apd, ctx, batch, pen, records)
            assert_dispatch(err[0], "record", case, swept)
            assert set(swept) == set(pairs)                                          # every pair has a window to record
            for p, record in enumerate(records):
                assert_window((paths[p], found[p], scores[p]), key, case.seqs, pen, record, kernel_id(case.kernel))
                if record[3] >= 1:
                    assert len(paths[p]) > 0 and path_ref.bits(paths[p]["cost"][-1:])[0] == path_ref.bits(costs[p])[0], record
    finally:
        batch.close()


@pytest.fixture(scope="module")
def register_rows():
    return kt.parse_spot_register_rows()


@pytest.mark.parametrize("kernel", REGISTER_KERNELS, ids=kernel_id)
def test_sweep_kernel_runs_and_matches_the_checker(apd, ctx, capfd, register_rows, kernel):
    sweep_case(apd, ctx, capfd, sm.register_case(*kernel), register_rows)


@pytest.mark.parametrize("kernel", REGISTER_KERNELS, ids=kernel_id)
def test_record_kernel_runs_and_matches_the_checker(apd, ctx, capfd, kernel):
    record_case(apd, ctx, capfd, sm.register_case(*kernel))


@pytest.mark.parametrize("dim", ANY_DIMENSIONS)
def test_sweep_of_a_dimension_without_kernels_of_its_own(apd, ctx, capfd, register_rows, dim):
    case = sm.any_case(dim)
    assert case.kernel == (0, 0) and len(case.tie_pairs) == 1
    sweep_case(apd, ctx, capfd, case, register_rows)


@pytest.mark.parametrize("dim", ANY_DIMENSIONS)
def test_record_of_a_dimension_without_kernels_of_its_own(apd, ctx, capfd, dim):
    record_case(apd, ctx, capfd, sm.any_case(dim))


def test_every_spotting_kernel_was_dispatched():
    """The union of the kernels' own lines over this module: every <RT, D> the header implies, as sweep and as record.  A case that
    silently stopped reaching its kernel fails here (and so does a run of this test without the cases above)."""
    want = {(kind,) + kernel for kind in kt.SPOT_KINDS for kernel in kt.spot_kernels()}
    assert _seen == want, "never dispatched: %r; not in the header: %r" % (sorted(want - _seen), sorted(_seen - want))
