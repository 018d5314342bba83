"""Ownership in the host layer: objects destroyed after their context, workspaces that grow and are reused on one context, and
the context's pair batch reused and replaced.  Results are compared with the CPU oracle by the rules of the neighbouring files:
assert_parity of tests/test_gpu_dtw.py (same 0 / +INF pattern, every finite distance within 1e-4 relative).
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_cross import assert_parity, config, oracle_cross, pack, walks

pytestmark = pytest.mark.gpu
F32P = C.POINTER(C.c_float)


def test_encoder_and_joined_batch_destroyed_after_their_context(apd):
    """apd_destroy releases the device side of every object still alive and orphans it; the object's own destroy call, made
    afterwards (the order a garbage collector may choose), frees the host part and returns APD_OK."""
    from audio_pattern_discovery_amd.alignments import Batch
    L = apd.lib()
    ctx = apd.Context(0)
    rng = np.random.default_rng(21)
    d_in, latent = 13, 8
    w = ((rng.random((d_in, latent)) - 0.5) / latent).astype(np.float32)
    b = ((rng.random(latent) - 0.5) / latent).astype(np.float32)
    enc = C.c_void_p()
    apd.check(L.apd_encoder_create(ctx.handle, w.ctypes.data_as(F32P), b.ctypes.data_as(F32P), d_in, latent, C.byref(enc)), ctx.handle)
    first = Batch(ctx, *pack(walks(("life", "a"), [9, 4, 7], 13), 13), 13)
    second = Batch(ctx, *pack(walks(("life", "b"), [5, 12], 13), 13), 13)
    joined = Batch.join(first, second)
    fs = np.zeros((3, 2), np.float32)
    cfg = config(0.5)
    apd.check(L.apd_align_cross(ctx.handle, joined.handle, C.byref(cfg), fs.ctypes.data_as(F32P), None), ctx.handle)   # plans cached
    ctx.close()
    assert L.apd_encoder_destroy(enc) == apd.APD_OK
    for batch in (joined, second, first):
        handle, batch.handle = batch.handle, None                    # the mirror's own close() must not free it a second time
        assert L.apd_batch_destroy(handle) == apd.APD_OK


def test_workspaces_grow_and_are_reused_on_one_context(apd, oracle):
    """The context's slab workspace serves a small batch, grows for a larger one, serves the small one again (no shrink), then a
    cross alignment of the two joined: one context, every result the oracle's."""
    from audio_pattern_discovery_amd.alignments import Batch
    L = apd.lib()
    ctx = apd.Context(0)
    rng = np.random.default_rng(22)
    small = walks(("grow", "small"), rng.integers(3, 10, size=5), 13)
    large = walks(("grow", "large"), rng.integers(20, 61, size=40), 13)
    cfg = config(0.0625)
    b_small, b_large = Batch(ctx, *pack(small, 13), 13), Batch(ctx, *pack(large, 13), 13)
    want = {id(b_small): oracle.align_all(*pack(small, 13), 0.0625, workers=8), id(b_large): oracle.align_all(*pack(large, 13), 0.0625, workers=8)}
    for batch in (b_small, b_large, b_small):
        n = batch.n_seq
        out = np.full((n, n), -7.0, np.float32)
        apd.check(L.apd_align_all(ctx.handle, batch.handle, C.byref(cfg), out.ctypes.data_as(F32P)), ctx.handle)
        assert_parity(out, want[id(batch)].reshape(n, n), "align_all of %d sequences" % n)
    joined = Batch.join(b_small, b_large)
    fs, sf = np.full((5, 40), -7.0, np.float32), np.full((40, 5), -7.0, np.float32)
    apd.check(L.apd_align_cross(ctx.handle, joined.handle, C.byref(cfg), fs.ctypes.data_as(F32P), sf.ctypes.data_as(F32P)), ctx.handle)
    want_fs, want_sf = oracle_cross(oracle, ("grow",), small, large, 13, 0.0625)
    assert_parity(fs, want_fs, "cross fs")
    assert_parity(sf, want_sf, "cross sf")
    for batch in (joined, b_large, b_small):
        batch.close()
    ctx.close()


def test_pair_batch_is_reused_and_replaced(apd, oracle):
    """apd_align_pair keeps the last pair's two-sequence batch: the same (n, m) again refills it, another shape replaces it."""
    from audio_pattern_discovery_amd.alignments import Alignment, AlignmentParams
    ctx = apd.Context(0)
    rng = np.random.default_rng(23)
    for n, m in [(7, 5), (7, 5), (9, 4)]:
        x = rng.standard_normal((n, 13)).astype(np.float32)
        y = rng.standard_normal((m, 13)).astype(np.float32)
        a = Alignment(ctx)
        a.construct_alignment(x, y, AlignmentParams(3, 0.8, 1.2, 1.0))
        assert_parity(np.array([a.score()]), np.array([oracle.dtw_pair(x, y, 3, 0.8, 1.2, 1.0)]), "pair %d x %d" % (n, m))
    ctx.close()
