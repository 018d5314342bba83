"""Inputs shared by the CPU twin tests (tests/test_oracle.py) and the GPU tests of the encoder and the VAT pre-segmentation
(tests/test_gpu_encoder.py, tests/test_gpu_vat.py): the exact-arithmetic VAT frames with their integer known answer, and
the encoder's weight regimes.  No GPU, no product code."""
import numpy as np

GRID_WRAP_FRAMES = 8192 * 256 + 300          # one more than the widest launch covers in a single pass (8192 blocks x 256 threads)

# ------------------------------------------------------------------------------------------------ VAT


def alternating(a, n_bins=4):
    """Frames [a, -a, a, -a, ...] (n_bins even): mean exactly 0, population std exactly |a| for small integers a."""
    a = np.asarray(a, dtype=np.float32)
    return np.ascontiguousarray(a[:, None] * np.where(np.arange(n_bins) % 2 == 0, 1, -1).astype(np.float32)[None, :])


def integer_ranges(a, k, idx, min_len):
    """spectrogram.rs:174-216 on alternating(a) in plain integers: k * variance[i] = sum(a[i-k:i]) (0 for i < k), the
    threshold is the idx-th smallest of them.  Returns (emitted ranges, runs closed but too short, first frame of the run still
    open at the end or None, the k-fold variances, the k-fold threshold)."""
    a = [abs(int(v)) for v in a]
    s = [sum(a[i - k:i]) if i >= k else 0 for i in range(len(a))]
    th = sorted(s)[idx]
    out, short, start, recording = [], [], 0, True
    for i, v in enumerate(s):
        if v >= th and not recording:
            start, recording = i, True
        if v < th and recording:
            recording = False
            (out if i - start > min_len else short).append((start, i))
    return out, short, (start if recording else None), s, th


# Written by hand for k = 4, perc = 0.5 (index 32 of 64), min_len = 3.  The 4-fold variances are
#   0 0 0 0 0 5 10 15 20 20 20 16 12 8 4 4 4 4 6 8 10 12 12 12 12 12 10 8 6 4 4 10 10 10 10 4 4 4 8 12 12 12 8 4 4 4 6 10 10 12
#   12 10 12 10 8 6 4 8 12 16 20 20 20 20,   threshold 10 (eleven values tied with it).
#  - frame 6 is the first at the threshold, through the window [2, 6) = 0 + 0 + 5 + 5; the window (2, 6] holds 15 and puts
#    the start at 5, the window [1, 5) holds 5 and puts it at 7;
#  - the lone 7 at frame 30 gives the run [31, 35) of four values all EQUAL to the threshold: length min_len + 1, emitted;
#  - the two 5s at 37, 38 give [39, 42): length min_len, closed but not emitted;
#  - the scan starts recording on the leading zeros and closes that run at frame 0 with length 0;
#  - the run that opens at 58 is still open at the end and is not emitted.
KAT_A = [0, 0, 0, 0, 5, 5, 5, 5, 5, 5, 1, 1, 1, 1, 1, 1, 1, 3, 3, 3, 3, 3, 3, 3, 3, 1, 1, 1, 1, 1, 7, 1, 1, 1, 1, 1, 1,
         5, 5, 1, 1, 1, 1, 1, 1, 3, 5, 1, 3, 3, 3, 3, 1, 1, 1, 1, 5, 5, 5, 5, 5, 5, 5, 5]
KAT_K, KAT_PERC, KAT_MIN_LEN = 4, 0.5, 3
KAT_RANGES = [(6, 13), (20, 27), (31, 35), (47, 54)]


def kat_frames():
    return alternating(KAT_A, 4)


def random_integer_a(t=500, seed=20261017):
    return np.random.default_rng(seed).integers(0, 9, t)


def wrap_a(t=GRID_WRAP_FRAMES, seed=5):
    """A slowly varying small integer: constant over 256 frames, so that a few thousand runs open and close.  The last
    three levels are set so that one run closes and another opens (and stays open) in the frames past 8192 * 256."""
    levels = np.random.default_rng(seed).integers(0, 9, t // 256 + 1)
    levels[-3:] = (8, 0, 8)
    return np.repeat(levels, 256)[:t]


# -------------------------------------------------------------------------------------------- encoder

# regime -> (weight scale: w, b uniform in +-scale/2; share of frames whose sigma is floored; max |pre-activation|)
# 0.125 = 1 / latent is Mat::seeded (numerics.rs:178-186).  expf(88.73) overflows f32, expf(-87.4) is subnormal.
REGIMES = {
    "seeded":      (0.125, (0.0, 0.0), (1.0, 3.0)),
    "floored":     (0.002, (1.0, 1.0), (0.0, 0.05)),
    "straddling":  (0.006, (0.3, 0.7), (0.0, 0.2)),
    "saturated":   (7.0, (0.0, 0.02), (80.0, 110.0)),
    "overflowing": (12.0, (0.0, 0.03), (140.0, 200.0)),
}
CAP = 1e-4                                   # no regime is allowed more than this, whatever the measurement says


def regime_inputs(name, t=4096, d_in=13, latent=8, seed=20261017):
    scale = np.float32(REGIMES[name][0])
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((t, d_in)) * 3).astype(np.float32)
    w = ((rng.random((d_in, latent)) - 0.5) * scale).astype(np.float32)
    b = ((rng.random(latent) - 0.5) * scale).astype(np.float32)
    return x, w, b


def regime_facts(enc, x, w, b):
    """(share of floored frames, min and max pre-activation), on the CPU.  A z-scored row has population std 1; a row whose
    sigma was floored at 1 (neural.rs:62) keeps its own, smaller one."""
    acc = x.astype(np.float64) @ w.astype(np.float64) + b.astype(np.float64)
    floored = float((enc.astype(np.float64).std(axis=1) < 0.999).mean())
    return floored, float(acc.min()), float(acc.max())


def check_regime(name, enc, x, w, b):
    """The inputs are in the regime their name claims (a changed generator must not quietly turn every case into 'seeded')."""
    _, (f_lo, f_hi), (a_lo, a_hi) = REGIMES[name]
    floored, lo, hi = regime_facts(enc, x, w, b)
    assert f_lo <= floored <= f_hi, (name, floored)
    assert a_lo <= max(-lo, hi) <= a_hi, (name, lo, hi)
    if name == "overflowing":
        assert lo < -88.8 and hi > 88.8, (lo, hi)               # expf overflows on one side and underflows on the other
    if name == "saturated":
        assert min(-lo, hi) > 17.0                              # 1 + expf(-17) == 1 in f32: the sigmoid saturates on both sides
    return floored, lo, hi


def oracle_error(oracle, npr, x, w, b):
    """max |f32 oracle - float64 twin| over the finite entries; the NaN patterns must agree."""
    want32, want64 = oracle.encode(x, w, b), npr.encode64(x, w, b)
    assert np.array_equal(np.isnan(want32), np.isnan(want64))
    ok = ~np.isnan(want64)
    return (float(np.abs(want32[ok].astype(np.float64) - want64[ok]).max()) if ok.any() else 0.0), want32, want64


def allowance(oracle_err):
    """What a kernel may differ from the float64 twin by: four times what the f32 oracle itself does on the same input --
    the kernel performs the oracle's operations in the oracle's order, and its expf may differ from libm's by its documented
    2 ulp (1 ulp for libm), which reaches the output through v, mu and the division -- and never more than CAP."""
    return min(4.0 * oracle_err, CAP)
