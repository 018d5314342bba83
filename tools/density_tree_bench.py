#!/usr/bin/env python3
"""apd_density_tree on the seeded N x N matrices of tools/density_bench.py, uploaded once: min_pts = 1 (single
linkage, no core-distance pass) and 9, the library's own events (apd_last_kernel_ms, apd_density_tree_last_profile: core distances,
rounds with their count, final ordering), best of 5 with the spread.

    N = 4096    blobs in 8 dimensions around 64 centres plus a fifth of uniform background, 67 MB: in the Infinity Cache
    N = 16384   the same, 1.07 GB: HBM

Against two yardsticks.  One streaming read of the matrix at 6.3 TB/s (section 4.24's figure) per round.  And the two routes a caller
had without the call: the matrix copied out of HBM, the mutual reachability built in numpy and scipy.sparse.csgraph.minimum_spanning_tree
on it (if scipy imports; its weights are compared with the library's); and 64 eps settings -- the tree's own edge weights, thinned by
rank as density_sweep thins them -- through apd_density_clusters in groups of 8, whose core points and labels are compared with the
tree's cuts.  Prints ONE JSON line.

    python tools/density_tree_bench.py
    python tools/density_tree_bench.py --sizes 4096 --repeats 5
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIZES, STREAM_RATE, MIN_PTS = (4096, 16384), 6.3e12, (1, 9)


def measure(sizes, repeats, scipy_largest):
    import numpy as np

    from audio_pattern_discovery_amd import _lib
    from audio_pattern_discovery_amd.clustering import density, density_cut
    from density_bench import blobs

    try:
        from scipy.sparse.csgraph import minimum_spanning_tree
    except ImportError:
        minimum_spanning_tree = None

    ctx = _lib.Context(0)
    ctx.set_timing(True)
    L = _lib.lib()
    out = dict(stream_rate=STREAM_RATE, repeats=repeats, sizes={})
    for n in sizes:
        d = blobs(n)
        d_mat = ctx.upload(d)
        model_ms = d.nbytes / STREAM_RATE * 1e3
        entry = dict(matrix_bytes=int(d.nbytes), model_ms=model_ms, runs=[])
        bufs = [ctx.alloc(4 * n) for _ in range(4)]                          # core, edge_i, edge_j, weight
        n_edges, nans = C.c_uint32(0), C.c_uint64(0)

        def call(min_pts):
            t0 = time.perf_counter()
            _lib.check(L.apd_density_tree(ctx.handle, d_mat.at(), 1, n, 0, min_pts, *[b.at() for b in bufs], C.byref(n_edges), C.byref(nans)), ctx.handle)
            wall = (time.perf_counter() - t0) * 1e3
            phases, rounds = (C.c_float * 3)(), C.c_uint32(0)
            _lib.check(L.apd_density_tree_last_profile(ctx.handle, phases, C.byref(rounds)))
            return ctx.last_kernel_ms(), wall, list(phases), int(rounds.value)

        for min_pts in MIN_PTS:
            call(min_pts)                                                    # once before anything is timed
            runs = [call(min_pts) for _ in range(repeats)]
            best = min(runs, key=lambda r: r[0])
            names = ("core", "rounds", "ordering")
            e = int(n_edges.value)
            tree = (bufs[0].to_numpy(np.float32, n), bufs[1].to_numpy(np.uint32, e), bufs[2].to_numpy(np.uint32, e), bufs[3].to_numpy(np.float32, e))
            run = dict(min_pts=min_pts, edges=e, nans=int(nans.value), kernels_ms_best=best[0], kernels_ms_all=[r[0] for r in runs],
                       call_wall_ms_best=min(r[1] for r in runs), call_wall_ms_all=[r[1] for r in runs], rounds=best[3],
                       phases_ms_best={k: min(r[2][i] for r in runs) for i, k in enumerate(names)},
                       phases_ms_all={k: [r[2][i] for r in runs] for i, k in enumerate(names)})
            run["round_ms"] = run["phases_ms_best"]["rounds"] / max(best[3], 1)
            run["round_over_model"] = run["round_ms"] / model_ms
            print("n %d min_pts %d: %d rounds, %r" % (n, min_pts, best[3], run["phases_ms_best"]), file=sys.stderr, flush=True)

            # route 1: the matrix copied out, mutual reachability in numpy, scipy's minimum spanning tree
            t0 = time.perf_counter()
            copied = d_mat.to_numpy(np.float32, n * n).reshape(n, n)
            copy_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            sym = np.minimum(copied, copied.T)
            if min_pts > 1:
                np.fill_diagonal(sym, np.inf)
                core = np.partition(sym, min_pts - 2, axis=1)[:, min_pts - 2]
                sym = np.maximum(sym, np.maximum(core[:, None], core[None, :]))
            np.fill_diagonal(sym, 0.0)
            numpy_s = time.perf_counter() - t0
            old = dict(copy_out_ms=copy_s * 1e3, numpy_mutual_reachability_ms=numpy_s * 1e3)
            if minimum_spanning_tree is not None and n <= scipy_largest:
                t0 = time.perf_counter()
                mst = minimum_spanning_tree(sym.astype(np.float64))
                old["scipy_minimum_spanning_tree_ms"] = (time.perf_counter() - t0) * 1e3
                old["weights_equal"] = bool(np.array_equal(np.sort(mst.data), np.sort(tree[3].astype(np.float64))))
                old["total_ms"] = old["copy_out_ms"] + old["numpy_mutual_reachability_ms"] + old["scipy_minimum_spanning_tree_ms"]
            run["old_route_scipy"] = old
            del copied, sym

            # route 2: 64 eps settings through apd_density_clusters, eight per call
            eps = np.unique(tree[3])
            eps = eps[np.round(np.linspace(0, len(eps) - 1, min(64, len(eps)))).astype(np.int64)]
            t0 = time.perf_counter()
            (labels, counts), (kind, _, _) = density((d_mat.at(), n), eps, min_pts, ctx=ctx, on_device=True, details=True)
            many_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            cut_labels, cut_counts, cut_kind = density_cut(tree, eps, details=True)
            cut_s = time.perf_counter() - t0
            core_mask = kind == _lib.APD_DENSITY_CORE
            run["old_route_density_clusters"] = dict(settings=len(eps), wall_ms=many_s * 1e3, tree_cuts_wall_ms=cut_s * 1e3,
                                                     core_equal=bool(np.array_equal(core_mask, cut_kind == _lib.APD_DENSITY_CORE)),
                                                     labels_equal_on_core=bool(np.array_equal(labels[core_mask], cut_labels[core_mask])))
            entry["runs"].append(run)
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
    ap.add_argument("--scipy-largest", type=int, default=1 << 21, help="largest N handed to scipy (its tree of a dense 16384 x 16384 takes minutes)")
    args = ap.parse_args()
    print(json.dumps(measure(args.sizes, args.repeats, args.scipy_largest)), flush=True)


if __name__ == "__main__":
    main()
