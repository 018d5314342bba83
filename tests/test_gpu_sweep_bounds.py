"""Sweep bounds of the systolic kernels (csrc/dtw_systolic.h): the rows are sequence b of a pair (a < b, the shorter one: the
resident order is longest first), the columns sequence a, and the sweep stops at the macro-step that captures the result cell
(sweep_steps_needed, csrc/apd_internal.h).  What could go wrong is a transposed plane (score(x=a, y=b) stored where score(x=b,
y=a) belongs), a sweep cut before some pair's capture (the bound is the largest of a wavefront, of a workgroup in the shared-column
kernel), and a threshold test that lost its superset property (the column sequence's largest norm).

Three small batches, every geometry that holds them forced through apd_set_variant (G = 8, 16, 32 with C = 9, and the shared-column
twin of G = 16), three launch forms each, all against the CPU oracle:
  hybrid form, unit penalties: 1e-4 relative with identical zeros and +INF pattern (the suite's bound for the fast forms);
  strict mode: the oracle's bits, both triangles;
  penalties (ins 1.5, del 0.5, mat 1.0), difference form: the oracle's bits -- nearly every entry is directed there.
The shared-column code must also keep the bits of its DPP twin.  Batches 1 and 2 are only used once the oracle's own matrix has
at least 8 asymmetric pairs, so that a transposed plane cannot hide behind a symmetric matrix.
"""
import os

import numpy as np
import pytest

import _kernel_table as kt
from audio_pattern_discovery_amd import synth

RTOL = 1e-4
PCT = 0.0625
UNIT, DIRECTED = (1.0, 1.0, 1.0), (1.5, 0.5, 1.0)                 # (insertion, deletion, match)
SHARED, TWIN = 41609, 1609
CAPACITY = {809: 72, 1609: 144, 3209: 288, SHARED: 144}         # band offsets 2w + 1 a pair may have: G * C

_batches, _wants = {}, {}


def hand_made():
    """Batch 3, one tile of 16 sequences whose pairs end their sweeps at different macro-steps (band 6.25 %: w = max(band, gap) + 2):
    lengths 2, 3 and 17; two equal lengths with different content (38, 38); lengths one apart; an exact copy (the two of 70 frames:
    score exactly 0); and 38 against 70 frames, w = 34 = gap + 2: the result cell has band offset u* = 2w - 2 = 66 in lane
    66 // 9 = 7, the last of the ceil(69 / 9) = 8 active lanes, so nothing can be cut at the end of that sweep.  Within every
    4 x 4 sub-block the bands differ by at most 18, inside the shared-column ring's slack of 19.  The second row of four (59 .. 56)
    is placed so that, for every geometry, some wavefront's / workgroup's largest bound is 1 above a multiple of the unroll: a bound
    one macro-step short would drop a whole block there and lose that pair's capture.  (test_what_the_batches_claim holds all this.)"""
    rng = np.random.default_rng(606)
    lens = [70, 69, 68, 59, 58, 57, 56, 39, 38, 38, 37, 17, 5, 3, 2]
    rng.shuffle(lens)
    seqs = [np.cumsum(rng.standard_normal((n, 13)), axis=0).astype(np.float32) * np.float32(0.3) for n in lens]
    seqs.insert(4, seqs[lens.index(70)].copy())
    return seqs


def batch(name):
    """(sequences, frames, offsets, lengths) of a batch, made once."""
    if name not in _batches:
        if name == "ragged":                                     # Batch 1: lengths 73 .. 115, |n - m| binds w for many pairs
            seqs = synth.split(*synth.make_sequences(24, 96, 13, seed=3, jitter=24))
        elif name == "even":                                     # Batch 2: lengths 194 .. 206, the band binds
            seqs = synth.split(*synth.make_sequences(16, 200, 13, seed=7, jitter=6))
        else:
            seqs = hand_made()
        lens = [len(s) for s in seqs]
        offsets = np.zeros(len(seqs) + 1, np.uint64)
        offsets[1:] = np.cumsum(lens)
        _batches[name] = (seqs, np.concatenate(seqs, axis=0).astype(np.float32), offsets, lens)
    return _batches[name]


def tile_needs(lens, pct):
    """2w + 1 per tile with the tile plan's bound of w (plan_tile_classes: resident order is longest first, 16 sequences per tile
    row, w = max(min(band, longest), longest - shortest) + 2 over the two rows of a tile)."""
    order = sorted(lens, reverse=True)
    rows = [order[i:i + 16] for i in range(0, len(order), 16)]
    needs = []
    for x in range(len(rows)):
        for y in range(x, len(rows)):
            mx, mn = max(rows[x][0], rows[y][0]), min(rows[x][-1], rows[y][-1])
            band = int(np.float32(pct) * np.float32(mx))
            needs.append(2 * (max(min(band, mx), mx - mn) + 2) + 1)
    return needs


C, U, SLACK = 9, 10, 19                                          # cells per lane, unroll (macro-steps per block), ring slack in w


def pair_w(n, m, pct=PCT):
    """w of one pair (pair_w, csrc/dtw_common.h)."""
    mx = max(n, m)
    return max(min(int(np.float32(pct) * np.float32(mx)), mx), abs(n - m)) + 2


def steps_needed(rows, cols):
    """sweep_steps_needed (csrc/apd_internal.h): the capture step of the result cell, plus one."""
    return (rows - 1) + ((cols - 1) - (rows - 1) + pair_w(rows, cols)) // C + 1


def sweep_groups(lens, code):
    """The pairs (len a, len b) that share a loop bound under `code`, one list per wavefront (DPP window: one b, 64 / G consecutive
    a) or per workgroup (shared columns: a 4 x 4 sub-block), in resident order; pairs that are not swept are left out."""
    order = sorted(lens, reverse=True)
    n, tiles, out = len(order), (len(order) + 15) // 16, []
    for ta in range(tiles):
        for tb in range(ta, tiles):
            if code == SHARED:
                cells = [[(sa + i, sb + j) for i in range(4) for j in range(4)] for sa in range(0, 16, 4) for sb in range(0, 16, 4)]
            else:
                ppw = 64 // (code // 100)
                cells = [[(a0 + i, b) for i in range(ppw)] for b in range(16) for a0 in range(0, 16, ppw)]
            for cell in cells:
                pairs = [(order[ta * 16 + a], order[tb * 16 + b]) for a, b in cell
                         if ta * 16 + a < tb * 16 + b < n and order[ta * 16 + a] >= 2 and order[tb * 16 + b] >= 2]
                if pairs:
                    out.append(pairs)
    return out


def want_for(oracle, name, pens):
    """The oracle's matrix, computed once per (batch, penalties) and never modified."""
    if (name, pens) not in _wants:
        _, frames, offsets, _ = batch(name)
        want = oracle.align_all(frames, offsets, PCT, *pens, workers=8)
        want.setflags(write=False)
        _wants[(name, pens)] = want
    return _wants[(name, pens)]


def run(ctx, name, pens, mode, variant, capfd):
    """(matrix, {geometry code: tiles}) of one alignment of the batch with `variant` forced."""
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery
    seqs = batch(name)[0]
    n = len(seqs)
    ctx.set_distance_mode(mode)
    ctx.set_variant(variant)
    os.environ["APD_DEBUG_PLAN"] = "1"
    try:
        capfd.readouterr()
        out = AlignmentWorkers.new([NDSequence(s) for s in seqs], ctx).align_all(
            Discovery(warping_band_percentage=PCT, insertion_penalty=pens[0], deletion_penalty=pens[1],
                      match_penalty=pens[2])).reshape(n, n).copy()
        plan = kt.read_plan(capfd.readouterr().err)
    finally:
        os.environ.pop("APD_DEBUG_PLAN", None)
        ctx.set_variant(0)
        ctx.set_distance_mode("hybrid")
    return out, plan


def assert_parity(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got)), what + ": INF/NaN pattern differs"
    assert np.array_equal(np.isposinf(want), np.isposinf(got)), what
    zero = fin & (want == 0)
    assert np.all(got[zero] == 0), what + ": exact zeros (diagonal, identical sequences) must stay 0"
    nz = fin & ~zero
    rel = np.abs(got[nz] - want[nz]) / np.abs(want[nz])
    print("%s: max rel err %.3e over %d entries" % (what, rel.max(), int(nz.sum())))
    assert rel.max() <= RTOL, "%s: max rel err %.3e" % (what, rel.max())


def assert_same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape
    differing = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print("%s: %d of %d entries differ bitwise" % (what, differing, got.size))
    assert differing == 0, "%s: %d of %d entries differ bitwise" % (what, differing, got.size)


def asymmetric_pairs(m):
    m = np.asarray(m, np.float32)
    return int((np.triu(m.view(np.uint32) != m.T.copy().view(np.uint32), 1)).sum())


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    c.set_distance_mode("hybrid")
    yield c
    c.set_variant(0)
    c.close()


# every geometry whose capacity holds every tile of the batch; the shared-column code wherever its DPP twin holds it
CASES = [(name, code) for name in ("ragged", "even", "hand-made") for code in (809, 1609, 3209, SHARED)
         if max(tile_needs(batch(name)[3], PCT)) <= CAPACITY[code]]


def test_the_cases_are_the_intended_ones():
    assert CASES == [("ragged", 1609), ("ragged", 3209), ("ragged", SHARED), ("even", 809), ("even", 1609), ("even", 3209),
                     ("even", SHARED), ("hand-made", 1609), ("hand-made", 3209), ("hand-made", SHARED)]
    lens = sorted(batch("hand-made")[3])
    assert lens[:3] == [2, 3, 5] and 17 in lens and lens.count(38) == 2 and lens.count(70) == 2 and len(lens) == 16
    assert (min(batch("ragged")[3]), max(batch("ragged")[3])) == (73, 115)


def test_what_the_batches_claim():
    """The properties the batches are chosen for, from their lengths alone."""
    # the loop bound is the group's largest sweep_steps_needed rounded up to U: a bound one too small changes the number of blocks,
    # and loses the capture of the pair that sets it, only where that maximum is 1 above a multiple of U
    for name, code in CASES:
        tops = [max(steps_needed(lb, la) for la, lb in g) for g in sweep_groups(batch(name)[3], code)]
        assert (name, code) == ("even", SHARED) or any(t % U == 1 for t in tops), (name, code, sorted(set(t % U for t in tops)))
    lens = batch("hand-made")[3]
    w = pair_w(38, 70)
    ustar = (70 - 1) - (38 - 1) + w
    assert w == 34 == (70 - 38) + 2 and ustar == 2 * w - 2 and ustar // C == (2 * w + 1 + C - 1) // C - 1    # the last active lane
    assert steps_needed(38, 70) == (38 - 1) + (2 * w + 1 + C - 1) // C                                       # nothing cut at the end
    tops = [[steps_needed(lb, la) for la, lb in g] for g in sweep_groups(lens, SHARED)]
    assert any(max(t) - min(t) >= U for t in tops)               # pairs of one workgroup end more than a block apart
    for name in ("ragged", "even", "hand-made"):                 # every workgroup within the shared-column ring's slack
        spreads = [max(ws) - min(ws) for ws in ([pair_w(la, lb) for la, lb in g] for g in sweep_groups(batch(name)[3], SHARED))]
        assert max(spreads) <= SLACK, (name, max(spreads))
    assert max(max(ws) - min(ws) for ws in ([pair_w(la, lb) for la, lb in g] for g in sweep_groups(lens, SHARED))) == 18


@pytest.mark.gpu
@pytest.mark.parametrize("name,code", CASES, ids=["%s-%d" % c for c in CASES])
def test_forced_geometry_matches_the_oracle_in_every_form(ctx, oracle, capfd, name, code):
    lens = batch(name)[3]
    n_tiles = len(tile_needs(lens, PCT))
    want = want_for(oracle, name, UNIT)
    if name != "hand-made":
        assert asymmetric_pairs(want) >= 8, "the oracle's matrix is too symmetric to show a transposed plane"
    else:                                                        # the exact copy, and the pair whose result cell is in the last active lane
        seqs = batch(name)[0]
        i, j = [k for k, s in enumerate(seqs) if len(s) == 70]
        assert np.array_equal(seqs[i], seqs[j]) and want[i, j] == 0.0 and want[j, i] == 0.0
    # hybrid form, unit penalties
    got, plan = run(ctx, name, UNIT, "hybrid", code, capfd)
    assert plan == {code: n_tiles}, "%s: the plan is %r, not every tile on %d" % (name, plan, code)
    assert_parity(got, want, "%s %d hybrid" % (name, code))
    if code == SHARED:
        twin, plan_t = run(ctx, name, UNIT, "hybrid", TWIN, capfd)
        assert plan_t == {TWIN: n_tiles}, plan_t
        assert_same_bits(got, twin, "%s shared columns against the DPP twin" % name)
    # strict mode and directed penalties: the plan names the shared-column class for neither, its tiles take the DPP twin
    other = TWIN if code == SHARED else code
    got, plan = run(ctx, name, UNIT, "strict", code, capfd)
    assert plan == {other: n_tiles}, plan
    assert_same_bits(got, want, "%s %d strict" % (name, code))
    want_d = want_for(oracle, name, DIRECTED)
    assert asymmetric_pairs(want_d) >= 8
    got, plan = run(ctx, name, DIRECTED, "exact", code, capfd)
    assert plan == {other: n_tiles}, plan
    assert_same_bits(got, want_d, "%s %d penalties 1.5 / 0.5 / 1.0" % (name, code))
