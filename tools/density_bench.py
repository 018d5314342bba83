#!/usr/bin/env python3
"""apd_density_clusters on seeded N x N matrices that are uploaded once: eps from the k-distance curve of
apd_neighbors (k = 8, min_pts = 9), one setting (the median of the curve) and eight (its 0.1 .. 0.9 quantiles), the library's own
events (apd_last_kernel_ms, apd_density_last_profile: adjacency, degree, propagation with its round count, border), best of 5 with
the spread.

    N = 4096    blobs in 8 dimensions around 64 centres plus a fifth of uniform background, 67 MB: in the Infinity Cache
    N = 16384   the same, 1.07 GB: HBM

Against two yardsticks.  One streaming read of the matrix at 6.3 TB/s, which the adjacency pass is meant to approach.  And the route
a caller had without the call, for one setting: the matrix copied out of HBM, the same clustering in numpy (threshold, degrees, core
points, minimum-label propagation with pointer jumping over the edge list, the border rule), checked to give the library's labels;
scipy.sparse.csgraph.connected_components on the thresholded core matrix if scipy imports.  For scale only, apd_clustering (UPGMA) on the
same resident matrix at --upgma-percentile: it computes something else.  Prints ONE JSON line.

    python tools/density_bench.py
    python tools/density_bench.py --sizes 4096 --repeats 5
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES, STREAM_RATE, K = (4096, 16384), 6.3e12, 8


def blobs(n, seed=0, dims=8, n_centers=64, background=0.2):
    import numpy as np
    rng = np.random.default_rng(seed)
    n_bg = int(n * background)
    centers = rng.standard_normal((n_centers, dims)).astype(np.float32) * 4
    x = rng.standard_normal((n - n_bg, dims)).astype(np.float32) * 0.5 + centers[rng.integers(0, n_centers, n - n_bg)]
    x = np.concatenate([x, rng.uniform(-8, 8, (n_bg, dims)).astype(np.float32)])[rng.permutation(n)]
    sq = (x * x).sum(1)
    d = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * (x @ x.T), 0.0)).astype(np.float32)
    np.fill_diagonal(d, 0.0)
    return d


def host_route(d, eps, min_pts):
    """(labels, seconds per step): the contract in numpy, EITHER."""
    import numpy as np
    n = len(d)
    t = [time.perf_counter()]
    near = d <= np.float32(eps)
    adj = near | near.T
    adj[np.arange(n), np.arange(n)] = False
    degree = adj.sum(1)
    core = degree + 1 >= min_pts
    t.append(time.perf_counter())
    rows, cols = np.nonzero(adj & core[:, None] & core[None, :])
    labels = np.arange(n, dtype=np.int64)
    rounds = 0
    while True:
        rounds += 1
        new = labels.copy()
        np.minimum.at(new, rows, labels[cols])
        new = new[new]
        if np.array_equal(new, labels):
            break
        labels = new
    t.append(time.perf_counter())
    rows, cols = np.nonzero(adj & ~core[:, None] & core[None, :])
    seen = np.full(n, n, np.int64)
    np.minimum.at(seen, rows, labels[cols])
    border = seen < n
    labels[border] = seen[border]
    t.append(time.perf_counter())
    return labels.astype(np.uint32), dict(threshold_degree_s=t[1] - t[0], components_s=t[2] - t[1], border_s=t[3] - t[2], rounds=rounds), adj, core


def measure(sizes, repeats, upgma_percentile):
    import numpy as np

    from audio_pattern_discovery_amd import _lib
    from audio_pattern_discovery_amd.clustering import neighbors

    try:
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        connected_components = None

    ctx = _lib.Context(0)
    ctx.set_timing(True)
    L = _lib.lib()
    f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    out = dict(stream_rate=STREAM_RATE, repeats=repeats, k=K, min_pts=K + 1, sizes={})
    for n in sizes:
        d = blobs(n)
        d_mat = ctx.upload(d)
        _, kth, _, _ = neighbors((d_mat.at(), n, n), K, skip_self=True, ctx=ctx, on_device=True)
        curve = kth[:, K - 1]
        model_ms = d.nbytes / STREAM_RATE * 1e3
        entry = dict(matrix_bytes=int(d.nbytes), model_ms=model_ms, runs=[])
        bufs = [ctx.alloc(4 * 8 * n), ctx.alloc(8 * n), ctx.alloc(4 * 8 * n), ctx.alloc(4 * 8 * 4), ctx.alloc(8)]

        def call(eps, min_pts):
            t0 = time.perf_counter()
            _lib.check(L.apd_density_clusters(ctx.handle, d_mat.at(), 1, n, 0, eps.ctypes.data_as(f32p), min_pts.ctypes.data_as(u32p), len(eps),
                                              *[b.at() for b in bufs]), ctx.handle)
            wall = (time.perf_counter() - t0) * 1e3
            phases, rounds = (C.c_float * 4)(), C.c_uint32(0)
            _lib.check(L.apd_density_last_profile(ctx.handle, phases, C.byref(rounds)))
            return ctx.last_kernel_ms(), wall, list(phases), int(rounds.value)

        for quantiles in ((0.5,), tuple(np.linspace(0.1, 0.9, 8))):
            eps = np.ascontiguousarray(np.quantile(curve, quantiles).astype(np.float32))
            min_pts = np.full(len(eps), K + 1, np.uint32)
            call(eps, min_pts)                                               # once before anything is timed
            runs = [call(eps, min_pts) for _ in range(repeats)]
            counts = bufs[3].to_numpy(np.uint32, 4 * len(eps)).reshape(len(eps), 4)
            best = min(runs, key=lambda r: r[0])
            names = ("adjacency", "degree", "propagation", "border")
            entry["runs"].append(dict(settings=len(eps), eps=[float(e) for e in eps], counts=counts.tolist(),
                                      kernels_ms_best=best[0], kernels_ms_all=[r[0] for r in runs], call_wall_ms_best=min(r[1] for r in runs),
                                      call_wall_ms_all=[r[1] for r in runs], rounds=best[3],
                                      phases_ms_best={k: min(r[2][i] for r in runs) for i, k in enumerate(names)},
                                      phases_ms_all={k: [r[2][i] for r in runs] for i, k in enumerate(names)},
                                      adjacency_over_model=min(r[2][0] for r in runs) / model_ms, kernels_over_model=best[0] / model_ms))
            print("n %d settings %d: %r" % (n, len(eps), entry["runs"][-1]["phases_ms_best"]), file=sys.stderr, flush=True)

        # the route a caller had, one setting
        eps = np.ascontiguousarray(np.quantile(curve, (0.5,)).astype(np.float32))
        call(eps, np.full(1, K + 1, np.uint32))
        ours = bufs[0].to_numpy(np.uint32, n)
        t0 = time.perf_counter()
        copied = d_mat.to_numpy(np.float32, n * n).reshape(n, n)
        copy_s = time.perf_counter() - t0
        labels, steps, adj, core = host_route(copied, eps[0], K + 1)
        old = dict(copy_out_ms=copy_s * 1e3, numpy_ms={k: (v * 1e3 if k != "rounds" else v) for k, v in steps.items()},
                   labels_equal=bool(np.array_equal(labels, ours)))
        old["total_ms"] = copy_s * 1e3 + sum(v for k, v in old["numpy_ms"].items() if k != "rounds")
        if connected_components is not None:
            t0 = time.perf_counter()
            graph = csr_matrix(adj & core[:, None] & core[None, :])
            n_comp, _ = connected_components(graph, directed=False)
            old["scipy_connected_components_ms"] = (time.perf_counter() - t0) * 1e3
            old["scipy_components_of_core_points"] = int(n_comp - (~core).sum())
        entry["old_route_one_setting"] = old
        del copied, adj

        ops = (_lib.ClusterOp * n)()
        roots = np.zeros(n, np.uint32)
        n_ops, n_roots, thr = C.c_uint32(0), C.c_uint32(0), C.c_float(0)
        t0 = time.perf_counter()
        _lib.check(L.apd_clustering(ctx.handle, d_mat.at(), 1, n, upgma_percentile, ops, C.byref(n_ops), roots.ctypes.data_as(u32p),
                                    C.byref(n_roots), C.byref(thr)), ctx.handle)
        entry["for_scale_upgma_another_computation"] = dict(percentile=upgma_percentile, wall_ms=(time.perf_counter() - t0) * 1e3, merges=int(n_ops.value))
        out["sizes"][str(n)] = entry
        for b in bufs + [d_mat]:
            b.free()
        del d
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=list(SIZES))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--upgma-percentile", type=float, default=0.01)
    args = ap.parse_args()
    print(json.dumps(measure(args.sizes, args.repeats, args.upgma_percentile)), flush=True)


if __name__ == "__main__":
    main()
