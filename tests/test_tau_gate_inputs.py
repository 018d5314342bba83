"""What tests/test_gpu_tau_gate.py claims about its inputs, without a GPU: the share of cells each threshold sends through the
hybrid form's recompute, for every batch that module aligns, and that its case lists hold every instantiation the header implies."""
import numpy as np

import _kernel_table as kt
import test_gpu_kernel_matrix as km
import test_gpu_tau_gate as tg


def every_batch():
    """Every batch of steps 2 to 4, once (the kernel matrix caches them per key)."""
    seen = {}
    for fam, a, b, dim in tg.LIVE:
        for shape in tg.shapes_of(fam):
            batch = km.batch_for(fam, a, b, dim, shape)
            seen[batch.key] = batch
    for dim in tg.CROSS_DIMS:
        for batch in (tg.cross_batch(dim), tg.cross_banded_batch(dim)):
            seen[batch.key] = batch
    return list(seen.values())


def test_hit_shares_of_every_batch_at_the_three_thresholds():
    """tau_mid: between 30 % and 70 % of the sampled cross-sequence frame pairs fall below tau (|x|^2 + |y|^2) -- hits and misses
    interleave; 4: all of them; the default 1/64: fewer than 5 % -- what the kernel matrix sees of the gate."""
    batches = every_batch()
    assert len(batches) > 100
    worst = [1.0, 0.0, 0.0]
    for batch in batches:
        ratios = tg.gate_ratios(batch)
        assert len(ratios) == tg.SAMPLE and np.all(ratios >= 0) and ratios.max() <= 2.0 + 1e-12      # d^2 <= 2 (|x|^2 + |y|^2)
        mid, low = tg.hit_share(batch, tg.tau_mid(batch)), tg.hit_share(batch, kt.default_tau())
        assert 0.30 <= mid <= 0.70, (batch.key, tg.tau_mid(batch), mid)
        assert tg.hit_share(batch, tg.TAU_ALL) == 1.0, batch.key
        assert low < 0.05, (batch.key, low)
        assert kt.default_tau() < tg.tau_mid(batch) < 2.0, (batch.key, tg.tau_mid(batch))
        worst = [min(worst[0], mid), max(worst[1], mid), max(worst[2], low)]
    print("%d batches: share below tau_mid %.3f .. %.3f, below 1/64 at most %.4f" % (len(batches), *worst))


def test_the_dc_offset_batches_sit_wholly_below_the_default_tau_and_above_the_control():
    """The plumbing control's and the contract tests' batches: every cell recomputed at 1/64, hardly any at 2^-30."""
    batches = [tg.knob_batch()] + [tg.dc_batch(km.batch_for(*km.smallest(fam)[:3], km.smallest(fam)[3], "full")) for fam in kt.FAMILIES]
    for batch in batches:
        assert not kt.leaves_fast_range(batch.frames)
        assert tg.hit_share(batch, kt.default_tau()) == 1.0 and tg.hit_share(batch, tg.TAU_ALL) == 1.0, batch.key
        assert tg.hit_share(batch, tg.TAU_NONE) < 0.01, (batch.key, tg.hit_share(batch, tg.TAU_NONE))


def test_every_live_instantiation_is_a_case_at_both_thresholds():
    """The id lists come from kt.pairs(): a geometry added to csrc/apd_internal.h is a new case of steps 2 and 3."""
    geoms, dims = kt.parse_table()
    want = {(fam, a, b, d) for fam, lst in geoms.items() for a, b in lst for d in dims
            if kt.instantiated(fam, a, b, d) and kt.hybrid_live(fam, d)}
    assert set(tg.LIVE) == want and len(tg.LIVE) == len(want)
    for test, tag in ((tg.test_every_cell_recomputed_matches_the_oracle, "tau-all"), (tg.test_hits_and_misses_interleaved_match_the_oracle, "tau-mid")):
        mark = next(m for m in test.pytestmark if m.name == "parametrize")
        assert list(mark.args[1]) == tg.LIVE
        assert sorted(mark.kwargs["ids"]) == sorted(km.case_id(*p, tag) for p in want)
    for fam in kt.FAMILIES:                                       # each of the five bodies, at more than one dimension
        assert len({p[3] for p in tg.LIVE if p[0] == fam}) >= 2, fam


def test_the_cross_batches_reach_several_families_at_every_dimension():
    for dim in tg.CROSS_DIMS:
        full = tg.takers(tg.cross_batch(dim), dim, tg.CROSS_FAMILIES)
        assert {"systolic", "wide", "strip"} <= {g[0] for g in full}, dim
        assert ("shared" in {g[0] for g in full}) == any(p[0] == "shared" and p[3] == dim for p in tg.LIVE)
        banded = tg.takers(tg.cross_banded_batch(dim), dim, tg.BANDED_FAMILIES)
        assert {g[0] for g in banded} == set(tg.BANDED_FAMILIES), dim
