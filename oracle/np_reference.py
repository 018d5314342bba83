"""Independent second opinion for the C oracle (TEST INFRASTRUCTURE, small cases only).

A literal Python/numpy re-derivation of the reference recurrence that shares no code
with oracle/apd_oracle.c: the DP table is a dict keyed (i, j) exactly like the
reference's HashMap (alignments.rs:99-111), every scalar is an np.float32 so each
operation rounds once as in the Rust build.  PARITY UNPINNED (see apd_oracle.h).

The VAT pre-segmentation (variance, interesting_ranges) is re-derived the same way, as f32
array operations that round once each; the encoder has a float64 evaluation of the same
formula (encode64), the high-precision yardstick the f32 oracle and the kernels are measured with.
"""
import numpy as np

F = np.float32
INF = F(np.inf)


def euclidean(x, y):
    """numerics.rs:114-120"""
    d = F(0.0)
    with np.errstate(all="ignore"):
        for a, b in zip(x, y):
            t = F(a) - F(b)
            d = F(d + F(t * t))
        return F(np.sqrt(d))


U64_MAX = (1 << 64) - 1


def warping_band(pct, n_size):
    """discovery.rs:38-45 -- f32 product, saturating truncation (Rust `as usize`: NaN and negatives 0, anything at or beyond
    2^64, +INF included, usize::MAX)."""
    with np.errstate(all="ignore"):
        v = F(pct) * F(n_size)
    if np.isnan(v) or v <= 0:
        return 0
    if v >= F(2.0 ** 64):
        return U64_MAX
    return int(v)


def window(n, m, band):
    """alignments.rs:173 with the band clamped to max(n, m) first (oracle/apd_oracle.h, "the band's domain"): where the reference's
    usize arithmetic overflows, the band is the full matrix."""
    return max(min(int(band), max(n, m)), abs(n - m)) + 2


def dtw_pair(x, y, band, ins=1.0, dele=1.0, match=1.0):
    """alignments.rs:107-180 (Alignment::new, construct_alignment, score)."""
    x = np.asarray(x, dtype=F)
    y = np.asarray(y, dtype=F)
    n, m = len(x), len(y)
    ins, dele, match = F(ins), F(dele), F(match)
    sparse = {(0, 0): F(0.0)}                       # :109
    if n == 0 and m == 0:
        return INF                                  # :117-118
    w = window(n, m, band)                          # :173
    with np.errstate(all="ignore"):                 # 0 * INF, INF - INF, overflow: IEEE results, wanted as they are
        for i in range(1, n + 1):                       # :174
            for j in range(max(i - w, 1) if i > w else 1, min(i + w, m + 1)):   # :175
                d = euclidean(x[i - 1], y[j - 1])       # :137
                ms = sparse.get((i - 1, j - 1), INF)    # :139
                is_ = sparse.get((i - 1, j), INF)       # :144
                ds = sparse.get((i, j - 1), INF)        # :149
                if ds < ms and ds < is_:                # :153
                    node = F(ds + F(dele * d))
                elif is_ < ms and is_ < ds:             # :155
                    node = F(is_ + F(ins * d))
                else:
                    node = F(ms + F(match * d))         # :158
                sparse[(i, j)] = node                   # :177
        cell = sparse.get((n - 1, m - 1))               # :120
        if cell is None:
            return INF
        return F(cell / F(n + m))                       # :121


def align_all(seqs, band_pct, ins=1.0, dele=1.0, match=1.0):
    """alignments.rs:17-67"""
    n = len(seqs)
    out = np.zeros((n, n), dtype=F)
    for i in range(n):
        for j in range(n):
            if i != j:
                ln = max(len(seqs[i]), len(seqs[j]))
                out[i, j] = dtw_pair(seqs[i], seqs[j], warping_band(band_pct, ln), ins, dele, match)
    return out


def percentile(x, perc):
    """numerics.rs:125-133"""
    x = np.asarray(x, dtype=F).ravel()
    nf = F(len(x)) * F(perc)
    numbers = np.sort(x[~np.isnan(x)], kind="stable")
    return numbers[int(nf)]


def clustering(dist, n, perc):
    """clustering.rs:81-210, literal; HashSet order replaced by ascending ids."""
    d = np.asarray(dist, dtype=F).reshape(n, n)
    parents = list(range(n))
    threshold = percentile(d, perc)
    ops = []

    def root(i):
        while parents[i] != i:
            i = parents[i]
        return i

    n_clusters, distance = n, F(0.0)
    while n_clusters > 1 and distance < threshold:
        assign = [root(i) for i in range(n)]
        clusters = sorted(set(assign))
        best, pq = INF, (0, 0)
        for ci in clusters:
            for cj in clusters:
                if ci == cj:
                    continue
                sx, sy, acc = F(0), F(0), F(0)
                for a in range(n):
                    if assign[a] == ci:
                        sy = F(0)
                        for b in range(n):
                            if assign[b] == cj:
                                acc = F(acc + d[a, b])
                                sy = F(sy + F(1))
                        sx = F(sx + F(1))
                link = F(acc / F(sx * sy))
                if link < best:
                    best, pq = link, (ci, cj)
        p, q = pq
        k = len(parents)
        parents[p] = k
        parents[q] = k
        parents.append(k)
        n_clusters -= 1
        if p < n and q < n:
            op = "Sequence2Sequence"
        elif p >= n and q >= n:
            op = "Cluster2Cluster"
        elif p >= n and q < n:
            op = "Cluster2Sequence"
        else:
            op = "Sequence2Cluster"
        ops.append(dict(merge_i=p, merge_j=q, into=k, distance=float(best), operation=op))
        distance = best
    return ops, sorted(set(root(i) for i in range(n))), float(threshold)


def variance(frames, k):
    """spectrogram.rs:174-187 with mean / std of numerics.rs:12-29.  One f32 array operation per reference operation, the
    frames side by side: every bin is added in order, `powf(v - mu, 2.0)` is the single rounded product (v - mu) * (v - mu)
    (what the compiler makes of a constant exponent 2), the window is the k values BEFORE frame i, summed oldest first.
    k = 0 takes the mean of an empty slice: 0 / 0 = NaN in every frame."""
    f = np.asarray(frames, dtype=F)
    t, n_bins = f.shape
    k = int(k)
    with np.errstate(all="ignore"):
        mu = np.zeros(t, dtype=F)
        for c in range(n_bins):
            mu = mu + f[:, c]                                   # numerics.rs:14-16
        mu = mu / F(n_bins)                                     # :17
        sq = np.zeros(t, dtype=F)
        for c in range(n_bins):
            d = f[:, c] - mu
            sq = sq + d * d                                     # :25-27
        deltas = np.sqrt(sq / F(n_bins))                        # :28
        out = np.zeros(t, dtype=F)                              # spectrogram.rs:183, i < k
        if t > k:
            acc = np.zeros(t - k, dtype=F)
            for q in range(k):
                acc = acc + deltas[q:q + t - k]                 # deltas[i - k + q] for i = k .. t-1
            out[k:] = acc / F(k)
    assert mu.dtype == F and deltas.dtype == F and out.dtype == F
    return out


def interesting_ranges(frames, k, perc, min_len):
    """spectrogram.rs:192-216.  Raises IndexError where the reference panics (numerics.rs:132: the index, taken from the
    unfiltered length, is past the NaN-filtered vector -- an empty sequence, perc = 1, k = 0, too many NaN frames)."""
    var = variance(frames, k)
    th = float(percentile(var, perc))                           # :198
    ranges, start, recording = [], 0, True                      # :200-202
    for i, v in enumerate(var.tolist()):                        # f32 -> Python float is exact: the comparisons are the f32 ones
        if v >= th and not recording:                           # :204-207
            start, recording = i, True
        if v < th and recording:                                # :208-213
            recording = False
            if i - start > min_len:
                ranges.append((start, i))
    return ranges


def encode64(x, w, b):
    """neural.rs:55-71 evaluated in float64 on the f32 inputs: x.mul(w).add_col(b).sigmoid().scale(255), then every row
    z-scored with its own population mean and std, the std floored at 1 (f32::max ignores a NaN operand, as fmax does)."""
    x = np.asarray(x, dtype=F).astype(np.float64)
    w = np.asarray(w, dtype=F).astype(np.float64)
    b = np.asarray(b, dtype=F).astype(np.float64).reshape(1, -1)
    with np.errstate(all="ignore"):
        pred = 255.0 * (1.0 / (1.0 + np.exp(-(x @ w + b))))
        mu = pred.mean(axis=1, keepdims=True)
        sigma = np.fmax(np.sqrt(((pred - mu) ** 2).mean(axis=1, keepdims=True)), 1.0)
        return (pred - mu) / sigma
