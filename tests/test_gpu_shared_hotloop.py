"""The steady-state loop of dtw_fused_systolic_shared (variant 41609): how the row frame reaches its registers and how the ring
addresses are formed.

Neither changes a value, so every case compares the uint32 views of the forced shared-column class with those of the DPP-window
kernel (variant 1609) on the same batch, and asks for oracle parity at the suite's tolerance.  What the cases are chosen for:
  * several wraps of the 160-column ring and of the 64-row ring, and a spread of w inside the workgroups (block bases, fill offsets);
  * every residue of the ring slot mod 8 (the padding term of the column address): eight consecutive w;
  * the recompute branch at every position of the unrolled block, in runs and alone, with some cells replaced and others kept:
    since the row frame of the next macro-step is on its way when the branch is taken, the branch reads its own row once more
    from the ring -- in a block's first step the row that the previous block fetched.
"""
import os

import numpy as np
import pytest

from _kernel_table import read_plan

pytestmark = pytest.mark.gpu
RTOL = 1e-4
DPP, SHARED = 1609, 41609
PCT = 0.15


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    c.set_distance_mode("hybrid")
    yield c
    c.set_variant(0)
    c.close()


def host_w(n, m, pct=PCT):
    """apd_internal.h, host_w: the band in f32 as the library computes it."""
    mx, gap = max(n, m), abs(n - m)
    band = min(int(np.float32(pct) * np.float32(mx)), mx)
    return max(band, gap) + 2


def align(ctx, seqs, variant, capfd):
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery
    n = len(seqs)
    ctx.set_variant(variant)
    os.environ["APD_DEBUG_PLAN"] = "1"
    try:
        capfd.readouterr()
        out = AlignmentWorkers.new([NDSequence(s) for s in seqs], ctx).align_all(
            Discovery(warping_band_percentage=PCT)).reshape(n, n).copy()
        plan = read_plan(capfd.readouterr().err)
    finally:
        os.environ.pop("APD_DEBUG_PLAN", None)
        ctx.set_variant(0)
    return out, plan


def assert_parity(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got)), "INF/NaN pattern differs"
    assert np.array_equal(np.isposinf(want), np.isposinf(got))
    zero = fin & (want == 0)
    assert np.all(got[zero] == 0), "exact zeros (diagonal, identical sequences) must stay 0"
    nz = fin & ~zero
    rel = np.abs(got[nz] - want[nz]) / np.abs(want[nz])
    print("max rel err %.3e" % rel.max())
    assert rel.max() <= RTOL, "max rel err %.3e" % rel.max()


def check(ctx, oracle, capfd, seqs):
    """Shared columns forced against the DPP window forced: the same bits; oracle parity; every tile on the shared class."""
    frames = np.concatenate(seqs, axis=0).astype(np.float32)
    offsets = np.zeros(len(seqs) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    want = oracle.align_all(frames, offsets, PCT, 1.0, 1.0, 1.0, workers=8)
    shared, plan_s = align(ctx, seqs, SHARED, capfd)
    dpp, plan_d = align(ctx, seqs, DPP, capfd)
    side = (len(seqs) + 15) // 16
    assert plan_s == {SHARED: side * (side + 1) // 2}, plan_s     # the shared-column class took every tile
    assert plan_d == {DPP: side * (side + 1) // 2}, plan_d
    a, b = shared.view(np.uint32), dpp.view(np.uint32)
    print("%d of %d entries differ from the DPP kernel" % (int((a != b).sum()), a.size))
    assert np.array_equal(a, b), "%d entries differ from the DPP kernel" % int((a != b).sum())
    assert_parity(shared, want)
    return shared


def gaussian(rng, lens, dim):
    return [rng.standard_normal((int(n), dim)).astype(np.float32) for n in lens]


@pytest.mark.parametrize("dim", [13, 8, 10])
def test_ring_wraps_and_band_spread(ctx, oracle, capfd, dim):
    """40 sequences of 380 .. 420 frames: w = 59 .. 65, the sweep crosses the column ring (160) twice and the row ring (64) six
    times, and the pairs of one workgroup differ in w."""
    rng = np.random.default_rng(600 + dim)
    lens = rng.integers(380, 421, size=40)
    ws = {host_w(int(a), int(b)) for a in lens for b in lens}
    assert min(ws) >= 59 and max(ws) <= 65 and len(ws) >= 5, sorted(ws)
    check(ctx, oracle, capfd, gaussian(rng, lens, dim))


def test_every_padding_residue_of_the_column_slot(ctx, oracle, capfd):
    """The slot a lane reads first is 1 + 8 (gl + 1) - w mod 160: with eight consecutive w every residue mod 8 occurs, so the
    16 bytes behind every eighth frame are crossed at every step of the unrolled block.  The longest length of a pair sets w:
    lengths from 380 (w = 59) in steps that move 0.15 * length through 57 .. 64."""
    rng = np.random.default_rng(77)
    lens = [380 + (47 * i) // 39 for i in range(40)]              # 380 .. 427
    ws = {host_w(a, b) for a in lens for b in lens}
    assert set(range(59, 67)) <= ws, sorted(ws)
    rng.shuffle(lens)
    check(ctx, oracle, capfd, gaussian(rng, lens, 13))


def test_gate_hits_at_every_block_position(ctx, oracle, capfd):
    """Pairs whose cells fall under the gate's threshold: (s, s) and (s, s[k:]) for k = 1 .. 10 put exact-zero cells on a diagonal,
    k columns off for each k, so the branch is taken in every step of every block (first and last included) by some lane of the
    wave, run after run; (s, s + 1e-3 noise) replaces cells next to cells that are kept; a sequence that shares every third frame with s takes
    the branch in isolated steps (period 3 against blocks of 10: every position, with untaken steps on both sides); two unrelated
    sequences fill waves that never take it."""
    rng = np.random.default_rng(2024)
    s = rng.standard_normal((400, 13)).astype(np.float32)
    seqs = [s, s.copy()] + [s[k:].copy() for k in range(1, 11)]
    seqs.append(s + np.float32(1e-3) * rng.standard_normal(s.shape).astype(np.float32))
    third = rng.standard_normal(s.shape).astype(np.float32)
    third[::3] = s[::3]
    seqs.append(third)
    seqs += gaussian(rng, [397, 392], 13)
    got = check(ctx, oracle, capfd, seqs)
    assert got[0, 1] == 0.0 and got[1, 0] == 0.0                  # identical sequences: the exact form gives exactly 0
