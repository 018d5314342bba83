"""Checker for the cluster prototypes (include/apd.h, "cluster prototypes"): TEST INFRASTRUCTURE, no GPU, no code shared with the
product.

The two contracts -- apd_cluster_medoids and apd_barycenters -- restated in np.float32 operations that round once each, on top of
the warping-path checker (tests/_path_reference.py: `path`, `band_from_pct`).  A vector add or division below is one f32 operation
per component, which is what the contract asks for.
"""
import numpy as np

import _path_reference as ref

F = np.float32
INF = F(np.inf)
NONE = 0xFFFFFFFF


def medoids(d, sets):
    """(medoid uint32 [len(sets)], cost float32): per set, members ascending, cost(i) = ((((0 + d[i][j1]) + d[j1][i]) + d[i][j2]) +
    d[j2][i]) + ...; a scan of i ascending keeps a member only if its cost is strictly below the best so far, starting from +INF."""
    d = np.asarray(d, dtype=F)
    medoid, cost = np.full(len(sets), NONE, dtype=np.uint32), np.full(len(sets), INF, dtype=F)
    with np.errstate(all="ignore"):
        for k, s in enumerate(sets):
            members = sorted(int(v) for v in s)
            for i in members:
                c = F(0.0)
                for j in members:
                    c = F(c + d[i, j])
                    c = F(c + d[j, i])
                if c < cost[k]:
                    cost[k], medoid[k] = c, i
    return medoid, cost


def iterate(c, seqs, members, pct, pen):
    """One iteration for one set: (new barycenter, inertia, used)."""
    T, dim = c.shape
    sums, cnt = np.zeros((T + 1, dim), dtype=F), np.zeros(T + 1, dtype=np.int64)
    total, used = F(0.0), 0
    with np.errstate(all="ignore"):
        for s in sorted(int(v) for v in members):
            y = np.asarray(seqs[s], dtype=F)
            steps, score = ref.path(c, y, ref.band_from_pct(pct, max(T, len(y))), *pen)
            if len(steps) == 0 or steps[0]["op"] != ref.START:
                continue                                           # did not reach the origin: structural, NaN costs do not matter
            used += 1
            total = F(total + score)
            for st in steps:
                if st["op"] == ref.START:
                    continue
                t = int(st["i"])
                sums[t] = sums[t] + y[int(st["j"]) - 1]
                cnt[t] += 1
        new = c.copy()
        for t in range(1, T + 1):
            if cnt[t] > 0:
                new[t - 1] = sums[t] / F(cnt[t])
        inertia = F(total / F(used)) if used else INF
    return new, inertia, used


def barycenters(seqs, sets, init, pct, pen=(1.0, 1.0, 1.0), iterations=1):
    """(list of [T_k][dim] float32 arrays, inertia [iterations][len(sets)], used): apd_barycenters.  pen: (insertion, deletion, match)."""
    dim = np.asarray(seqs[0]).shape[1]
    out = []
    inertia, used = np.full((iterations, len(sets)), INF, dtype=F), np.zeros((iterations, len(sets)), dtype=np.uint32)
    for k, s in enumerate(sets):
        if len(s) == 0:
            out.append(np.zeros((0, dim), dtype=F))
            continue
        c = np.array(seqs[init[k]], dtype=F)
        for it in range(iterations):
            c, inertia[it, k], used[it, k] = iterate(c, seqs, s, pct, pen)
        out.append(c)
    return out, inertia, used
