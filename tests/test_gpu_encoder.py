"""The encoder kernels (encode_staged_kernel, encode_kernel; reference neural.rs:55-71) outside the one regime the rest of the
suite draws from: weight scales that floor sigma, straddle the floor, saturate the sigmoid and overflow expf; non-finite
frames; the staged / un-staged switch at its edge; degenerate dimensions; the weight limit; both grid-stride loops.

Yardstick.  The kernels are measured against neural.rs:55-71 evaluated in float64 (oracle/np_reference.encode64).  What they
may differ from it by is what the f32 C oracle itself differs from it by ON THE SAME INPUT, times 4, and never more than 1e-4
(_companion_cases.allowance): the kernel performs the oracle's operations in the oracle's order, so it shares the oracle's
rounding of v = 255 s, of mu and of sigma; the one operation that is not bit-identical is expf, documented to 2 ulp on the
device against 1 ulp for libm, and that difference reaches the output through v, mu and the division.  The oracle's own
figures for 4096 frames of 13 -> 8 (tests/test_oracle.py::test_encoder_oracle_against_float64_twin):

    seeded 4.35e-6   floored 2.83e-5   straddling 2.85e-5   saturated 2.79e-5   overflowing 2.99e-5

so the allowance is 1.7e-5 in the seeded regime and the 1e-4 cap in the other four (4 x 2.8e-5 .. 3.0e-5 = 1.1e-4 .. 1.2e-4
would exceed it: those errors are half-ulps of v near 127.5 and 255 and of a sum near 1020, which the kernel rounds exactly
as the oracle does, so the factor 4 is generous there and the cap costs nothing).  Against the oracle itself the seeded regime
keeps the suite's 1e-5."""
import ctypes as C
import time

import numpy as np
import pytest

import _companion_cases as cc
from oracle import np_reference as npr

pytestmark = pytest.mark.gpu
F32P = C.POINTER(C.c_float)
UNWRITTEN = 0xFFFFFFFF                       # device_fill(0xFF): a NaN no computation produces with this payload


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    yield c
    c.close()


def encode_call(apd, ctx, x_ptr, t, w, b, on_device, out_ptr):
    w = np.ascontiguousarray(w, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return apd.lib().apd_encode(ctx.handle, x_ptr, t, w.shape[0], w.ctypes.data_as(F32P), b.ctypes.data_as(F32P), w.shape[1],
                                on_device, out_ptr)


def encode_status(apd, ctx, x, w, b):
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros((x.shape[0], w.shape[1]), np.float32)
    return encode_call(apd, ctx, C.c_void_p(x.ctypes.data), x.shape[0], w, b, 0, C.c_void_p(out.ctypes.data)), out


def encode_host(apd, ctx, x, w, b):
    rc, out = encode_status(apd, ctx, x, w, b)
    apd.check(rc, ctx.handle)
    return out


def encode_device(apd, ctx, x, w, b, off):
    """Device arrays `off` floats past a 16-byte boundary, the output between two guard zones that must stay unwritten."""
    t, latent = x.shape[0], w.shape[1]
    d_x = ctx.alloc(4 * (x.size + 4))
    d_x.copy_from(np.ascontiguousarray(x, np.float32).ravel(), byte_offset=4 * off)
    lead = 4 + off
    d_z = ctx.alloc(4 * (lead + t * latent + 8))
    d_z.fill(0xFF)
    assert d_x.ptr % 16 == 0 and d_z.ptr % 16 == 0
    apd.check(encode_call(apd, ctx, d_x.at(4 * off), t, w, b, 1, d_z.at(4 * lead)), ctx.handle)
    ctx.synchronize()
    raw = d_z.to_numpy(np.uint32)
    assert np.all(raw[:lead] == UNWRITTEN) and np.all(raw[lead + t * latent:] == UNWRITTEN), "wrote outside its rows"
    return raw[lead:lead + t * latent].view(np.float32).reshape(t, latent)


def assert_close(got, want32, want64, tol, what=""):
    """NaN exactly where the oracle has NaN; everything else within tol of the float64 twin.  Returns the measured maximum."""
    nan = np.isnan(want32)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN pattern differs in rows %s" % (what, np.unique(np.nonzero(np.isnan(got) != nan)[0])[:8])
    if nan.all():
        return 0.0
    err = float(np.abs(got[~nan].astype(np.float64) - want64[~nan]).max())
    assert err <= tol, "%s: max |gpu - float64| = %.3e > %.3e" % (what, err, tol)
    return err


def seeded(rng, t, d_in, latent, sd=2.0):
    x = (rng.standard_normal((t, d_in)) * sd).astype(np.float32)
    w = ((rng.random((d_in, latent)) - 0.5) / latent).astype(np.float32)        # Mat::seeded (numerics.rs:178-186)
    b = ((rng.random(latent) - 0.5) / latent).astype(np.float32)
    return x, w, b


@pytest.mark.parametrize("regime", list(cc.REGIMES))
def test_weight_regimes(ctx, apd, oracle, regime):
    x, w, b = cc.regime_inputs(regime)
    o_err, want32, want64 = cc.oracle_error(oracle, npr, x, w, b)
    floored, lo, hi = cc.check_regime(regime, want32, x, w, b)
    tol = cc.allowance(o_err)
    assert 0 < tol <= cc.CAP
    got = encode_host(apd, ctx, x, w, b)
    err = assert_close(got, want32, want64, tol, regime)
    vs_oracle = float(np.abs(got.astype(np.float64) - want32).max())
    print("%s: floored %.3f, acc in [%.1f, %.1f]; oracle-f64 %.3e, allowance %.3e, gpu-f64 %.3e, gpu-oracle %.3e"
          % (regime, floored, lo, hi, o_err, tol, err, vs_oracle))
    if regime == "seeded":
        assert vs_oracle <= 1e-5
    if regime == "floored":                                                     # v - mu divided by exactly 1: the rows keep their own std
        assert got.astype(np.float64).std(axis=1).max() < 1.0
    # the same through device arrays one float off a 16-byte boundary (scalar loads and stores in the staged kernel)
    assert np.array_equal(encode_device(apd, ctx, x[:1000], w, b, 1).view(np.uint32), got[:1000].view(np.uint32))


# (d_in, latent): (50, 10) is the last shape staged through LDS (65 536 bytes), (51, 10) the first that is not;
# (127, 128) fills the 64 KiB weight limit exactly
SHAPES = [(13, 8), (50, 10), (51, 10), (61, 1), (1, 61), (1, 1), (127, 128)]


def staged_bytes(d_in, latent):
    return ((d_in * latent + latent + 3) & ~3) * 4 + 4 * 64 * ((d_in | 1) + (latent | 1)) * 4


def test_switch_edge_is_where_the_shapes_say():
    assert staged_bytes(50, 10) == 64 * 1024 and staged_bytes(51, 10) > 64 * 1024
    assert staged_bytes(61, 1) <= 64 * 1024 and staged_bytes(1, 61) <= 64 * 1024 and staged_bytes(32, 31) > 64 * 1024
    assert (127 * 128 + 128) * 4 == 64 * 1024 and (144 * 113 + 113) * 4 == 64 * 1024 + 4


def test_switch_edge_runs_the_kernel_the_shapes_say(ctx, apd, capfd):
    """Both kernels compute the same values, so only the APD_DEBUG_PLAN line tells which one a shape ran."""
    import os
    rng = np.random.default_rng(4)
    ran = {}
    os.environ["APD_DEBUG_PLAN"] = "1"
    capfd.readouterr()
    try:
        for d_in, latent in SHAPES + [(32, 31)]:
            encode_host(apd, ctx, *seeded(rng, 3, d_in, latent))
            lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[apd] encoder")]
            assert len(lines) == 1, lines
            assert lines[0].startswith("[apd] encoder %d -> %d: " % (d_in, latent))
            kind, rest = lines[0].split(": ")[1].split(", ")
            ran[(d_in, latent)] = (kind, int(rest.split()[0]))
    finally:
        os.environ.pop("APD_DEBUG_PLAN", None)
    for shape in SHAPES + [(32, 31)]:
        staged = staged_bytes(*shape) <= 64 * 1024
        assert ran[shape] == (("staged", staged_bytes(*shape)) if staged else ("direct", (shape[0] * shape[1] + shape[1]) * 4)), shape
    assert ran[(50, 10)] == ("staged", 65536) and ran[(51, 10)][0] == "direct" and ran[(127, 128)] == ("direct", 65536)


@pytest.mark.parametrize("d_in,latent", SHAPES)
def test_shapes_frame_counts_and_alignment(ctx, apd, oracle, d_in, latent):
    """Frame counts around the 64-frame chunk, aligned pointers and pointers one float off.  One input of 257 frames per shape;
    the shorter runs are its prefixes, and the allowance is the one measured on all 257 frames."""
    rng = np.random.default_rng(1000 * d_in + latent)
    x, w, b = seeded(rng, 257, d_in, latent)
    o_err, want32, want64 = cc.oracle_error(oracle, npr, x, w, b)
    tol = cc.allowance(o_err)
    if latent == 1:
        assert np.all(want32 == 0.0) and tol == 0.0                             # sigma = 0, floored: (v - v) / 1
    worst = 0.0
    for t in (1, 63, 64, 65, 257):
        for off in (0, 1):
            got = encode_device(apd, ctx, x[:t], w, b, off)
            worst = max(worst, assert_close(got, want32[:t], want64[:t], tol, "t=%d off=%d" % (t, off)))
        assert np.array_equal(encode_host(apd, ctx, x[:t], w, b).view(np.uint32), got.view(np.uint32))
    print("(%d, %d): oracle-f64 %.3e, allowance %.3e, gpu-f64 %.3e" % (d_in, latent, o_err, tol, worst))


def test_one_past_the_weight_limit_is_refused(ctx, apd):
    rng = np.random.default_rng(3)
    x, w, b = seeded(rng, 2, 144, 113)
    rc, out = encode_status(apd, ctx, x, w, b)
    assert rc == apd.APD_ERR_UNSUPPORTED and np.all(out == 0.0)
    enc = C.c_void_p()
    assert apd.lib().apd_encoder_create(ctx.handle, w.ctypes.data_as(F32P), b.ctypes.data_as(F32P), 144, 113, C.byref(enc)) == apd.APD_ERR_UNSUPPORTED
    assert not enc.value


def nonfinite_block(rng, t, d_in, latent):
    """Seeded weights with w[3][2] = 0, and frames holding NaN, +inf, -inf, inf against the zero weight (inf * 0 = NaN in the
    product) and two infinities of opposite sign; first and last lanes of a 64-frame chunk among them."""
    x, w, b = seeded(rng, t, d_in, latent)
    k3 = min(3, d_in - 1)
    w[k3, min(2, latent - 1)] = 0.0
    x[5, 0] = np.nan
    x[63, d_in - 1] = np.inf
    x[64, 0] = -np.inf
    x[100, k3] = np.inf                                                         # inf * 0
    x[127, 0] = np.nan
    x[128, d_in - 1] = np.nan
    x[200, 0], x[200, d_in - 1] = np.inf, -np.inf
    x[t - 1, 0] = np.inf
    return x, w, b


@pytest.mark.parametrize("d_in,latent", [(13, 8), (50, 10), (51, 10)])
def test_nonfinite_frames(ctx, apd, oracle, d_in, latent):
    """A NaN in the pre-activation makes the whole row NaN (mu is NaN; fmaxf(NaN, 1) = 1 as f32::max); an infinite
    pre-activation saturates to 0 or 255 and the row stays finite; the frames next to either are untouched."""
    rng = np.random.default_rng(d_in)
    t = 300
    x, w, b = nonfinite_block(rng, t, d_in, latent)
    o_err, want32, want64 = cc.oracle_error(oracle, npr, x, w, b)
    nan_rows = np.isnan(want32).all(axis=1)
    assert np.array_equal(np.isnan(want32).any(axis=1), nan_rows)               # a row is NaN entirely or not at all
    assert nan_rows[[5, 100, 127, 128]].all() and 4 <= nan_rows.sum() <= 7
    assert not nan_rows[[4, 6, 62, 65, 99, 101, 126, 129]].any()
    assert np.isfinite(want32[~nan_rows]).all() and (~nan_rows[[63, 64, t - 1]]).sum() >= 1
    tol = cc.allowance(o_err)
    clean = x.copy()
    clean[~np.isfinite(clean)] = 0.0
    for off in (0, 1):
        got = encode_device(apd, ctx, x, w, b, off)
        assert_close(got, want32, want64, tol, "off=%d" % off)
        # a frame without a non-finite value gives the bits it gives in a run without any
        same = np.isfinite(x).all(axis=1)
        assert np.array_equal(got[same].view(np.uint32), encode_device(apd, ctx, clean, w, b, off)[same].view(np.uint32))


def grid_wrap(ctx, apd, oracle, d_in, latent, nonfinite):
    """8192 * 256 + 300 frames: the launch is capped at 8192 blocks of 256 threads (= 4 chunks of 64), so the last 300 frames
    are the second iteration of the kernel's grid-stride loop.  The input repeats a block of 1021 frames (a prime: the block
    never lines up with a chunk or with the grid); frames are independent, so the output must repeat the block's output bit
    for bit, and the block's output is held to the usual yardstick."""
    rng = np.random.default_rng(d_in * 100 + latent)
    block = 1021
    t = cc.GRID_WRAP_FRAMES
    x, w, b = nonfinite_block(rng, block, d_in, latent) if nonfinite else seeded(rng, block, d_in, latent)
    o_err, want32, want64 = cc.oracle_error(oracle, npr, x, w, b)
    reps, rem = divmod(t, block)
    tiled = np.concatenate([np.tile(x, (reps, 1)), x[:rem]])
    assert tiled.shape == (t, d_in)
    d_x, d_z = ctx.upload(tiled), ctx.alloc(4 * t * latent)
    del tiled
    d_z.fill(0xFF)
    ctx.synchronize()
    t0 = time.perf_counter()
    rc = encode_call(apd, ctx, d_x.at(), t, w, b, 1, d_z.at())
    apd.check(rc, ctx.handle)
    ctx.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    got = d_z.to_numpy(np.uint32).reshape(t, latent)
    d_x.free()
    d_z.free()
    first = got[:block]
    assert np.array_equal(np.isnan(first.view(np.float32)), np.isnan(want32)), "NaN pattern of the first block differs"
    assert (got[:reps * block].reshape(reps, block, latent) == first[None]).all(), "a later block differs from the first"
    assert np.array_equal(got[reps * block:], first[:rem]), "the frames of the second loop iteration differ"
    err = assert_close(first.view(np.float32), want32, want64, cc.allowance(o_err), "first block")
    print("(%d, %d) x %d frames: apd_encode on device arrays %.1f ms; oracle-f64 %.3e, gpu-f64 %.3e" % (d_in, latent, t, ms, o_err, err))


def test_unstaged_grid_wrap(ctx, apd, oracle):
    """(32, 31) is the cheapest shape encode_kernel is chosen for: 268 MB in, 260 MB out."""
    assert staged_bytes(32, 31) > 64 * 1024
    grid_wrap(ctx, apd, oracle, 32, 31, nonfinite=False)


def test_staged_grid_wrap_with_nonfinite_frames(ctx, apd, oracle):
    """The staged kernel's second iteration reuses the wavefront's LDS rows: rows that held a NaN or an infinite frame in
    the first chunk must not leak into the frames of the second, nor the other way round."""
    assert staged_bytes(13, 8) <= 64 * 1024
    grid_wrap(ctx, apd, oracle, 13, 8, nonfinite=True)
