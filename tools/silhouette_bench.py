#!/usr/bin/env python3
"""apd_silhouette on seeded N x N matrices that are uploaded once: one UPGMA run, 16 cuts of its dendrogram
between the 0.01 and the 0.5 percentile, both axes, the library's own events (apd_last_kernel_ms), best of 5 with the spread.

    N = 4096    blobs in 8 dimensions around 64 centres (the stand-in of tools/upgma_scale.py), 67 MB: in the Infinity Cache
    N = 16384   the same blobs, 1.07 GB: HBM

Against the route a caller has without it, in the same process and taking turns with the new call, per cut: apd_cross_linkage on the
resident matrix with every cluster of the cut as a set (singletons as sets of one; ROWS reads link_fs, COLUMNS link_sf), the [n][K]
linkage matrix copied out, a, b and s in numpy (the own cluster's column rescaled from the diagonal-inclusive mean, which is NOT the
contract's chain -- the route is timed, not checked bitwise).  --baseline-cuts limits that route to that many cuts spread over the list
and scales it.  And against one streaming read of the matrix at 6.3 TB/s.  Also reports the longest chain (the largest cluster of any cut)
and the time of a call with that cut alone.  Prints ONE JSON line.

    python tools/silhouette_bench.py
    python tools/silhouette_bench.py --sizes 4096 --repeats 5 --baseline-cuts 16
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES, CUTS, STREAM_RATE = (4096, 16384), 16, 6.3e12


def blobs(n, seed=0, dims=8, n_centers=64):
    import numpy as np
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dims)).astype(np.float32) * 0.5 + (rng.standard_normal((n_centers, dims)).astype(np.float32) * 4)[rng.integers(0, n_centers, n)]
    sq = (x * x).sum(1)
    d = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * (x @ x.T), 0.0)).astype(np.float32)
    np.fill_diagonal(d, 0.0)
    return d


def measure(sizes, repeats, baseline_cuts, lo, hi):
    import numpy as np

    from audio_pattern_discovery_amd import _lib
    from audio_pattern_discovery_amd.clustering import AgglomerativeClustering, ClusteringOperation, Merge

    ctx = _lib.Context(0)
    ctx.set_timing(True)
    L = _lib.lib()
    u32p = C.POINTER(C.c_uint32)
    out = dict(stream_rate=STREAM_RATE, repeats=repeats, cuts=CUTS, percentiles=[lo, hi], sizes={})
    for n in sizes:
        d = blobs(n)
        d_mat = ctx.upload(d)
        ops = (_lib.ClusterOp * n)()
        roots = np.zeros(n, np.uint32)
        n_ops, n_roots, thr = C.c_uint32(0), C.c_uint32(0), C.c_float(0)
        t0 = time.perf_counter()
        _lib.check(L.apd_clustering(ctx.handle, d_mat.at(), 1, n, hi, ops, C.byref(n_ops), roots.ctypes.data_as(u32p), C.byref(n_roots),
                                    C.byref(thr)), ctx.handle)
        upgma_s = time.perf_counter() - t0
        operations = [ClusteringOperation(o.merge_i, o.merge_j, o.into, o.distance, Merge(o.operation)) for o in ops[:n_ops.value]]
        percs = np.exp(np.linspace(np.log(lo), np.log(hi), CUTS))
        t0 = time.perf_counter()
        labels = np.zeros((CUTS, n), np.uint32)
        kept = []
        for c, p in enumerate(percs):
            v = C.c_float(0)
            _lib.check(L.apd_percentile(ctx.handle, d_mat.at(), n * n, float(p), 1, C.byref(v)), ctx.handle)
            kept.append(len(AgglomerativeClustering.cut(operations, v.value)))
            labels[c] = AgglomerativeClustering.assignment(operations[:kept[c]], n)
        cuts_s = time.perf_counter() - t0
        sizes_of = [np.unique(lab, return_counts=True)[1] for lab in labels]
        longest_cut = int(np.argmax([s.max() for s in sizes_of]))
        per_cut = [ctx.alloc(4 * CUTS) for _ in range(3)]
        per_sample = [ctx.alloc(4 * CUTS * n) for _ in range(4)]
        entry = dict(matrix_bytes=int(d.nbytes), upgma_s=upgma_s, percentiles_cuts_labels_s=cuts_s, kept=kept,
                     clusters=[int(len(s)) for s in sizes_of], largest_cluster=[int(s.max()) for s in sizes_of], runs=[])

        def call(lab, axis):
            t0 = time.perf_counter()
            _lib.check(L.apd_silhouette(ctx.handle, d_mat.at(), 1, n, axis, lab.ctypes.data_as(u32p), len(lab), *[b.at() for b in per_cut],
                                        *[b.at() for b in per_sample]), ctx.handle)
            ms = ctx.last_kernel_ms()                                       # waits for the call's last event
            return ms, (time.perf_counter() - t0) * 1e3

        def old_route(lab, axis):
            """(s [n], seconds): what a caller does at the parent commit for one cut."""
            t0 = time.perf_counter()
            present, inverse, counts = np.unique(lab, return_inverse=True, return_counts=True)
            order = np.argsort(lab, kind="stable").astype(np.uint32)
            set_off = np.zeros(len(present) + 1, np.uint32)
            set_off[1:] = np.cumsum(counts)
            K = len(present)
            link = [ctx.alloc(4 * n * K), ctx.alloc(4 * n * K)]
            near = [ctx.alloc(4 * n), ctx.alloc(4 * n)]
            try:
                _lib.check(L.apd_cross_linkage(ctx.handle, d_mat.at(), d_mat.at(), 1, n, n, order.ctypes.data_as(u32p), set_off.ctypes.data_as(u32p),
                                               K, link[0].at(), link[1].at(), near[0].at(), near[1].at()), ctx.handle)
                mean = link[axis].to_numpy(np.float32, n * K).reshape(n, K)  # the copy waits for the stream
            finally:
                for b in link + near:
                    b.free()
            me = np.arange(n)
            own_cnt = counts[inverse].astype(np.float32)
            diag = d[me, me]
            with np.errstate(all="ignore"):
                a = np.where(own_cnt > 1, (mean[me, inverse] * own_cnt - diag) / (own_cnt - 1), 0).astype(np.float32)
                mean[me, inverse] = np.inf
                b = mean.min(axis=1)
                s = np.where(own_cnt > 1, (b - a) / np.maximum(a, b), 0)
            return s, time.perf_counter() - t0

        for axis in (0, 1):
            call(labels, axis)                                              # once before anything is timed
            new_ms, new_wall, old_s = [], [], []
            for r in range(repeats):                                        # the new call and today's route take turns
                ms, wall = call(labels, axis)
                new_ms.append(ms)
                new_wall.append(wall)
                timed = range(0, CUTS, CUTS // baseline_cuts)                # spread over the list: the cuts differ in their cluster counts
                old_s.append(sum(old_route(labels[c], axis)[1] for c in timed) * CUTS / len(timed))
                print("n %d axis %d repeat %d: new %.3f ms, old route %.1f ms" % (n, axis, r, ms, old_s[-1] * 1e3), file=sys.stderr, flush=True)
            s_new = per_sample[0].to_numpy(np.float32, CUTS * n).reshape(CUTS, n)[0]
            s_old = old_route(labels[0], axis)[0]
            alone = [call(labels[longest_cut:longest_cut + 1], axis)[0] for _ in range(repeats)]
            model_ms = d.nbytes * (1 if axis == 0 else 3) / STREAM_RATE * 1e3
            entry["runs"].append(dict(axis=("rows", "columns")[axis], kernels_ms_best=min(new_ms), kernels_ms_all=new_ms,
                                      call_wall_ms_best=min(new_wall), call_wall_ms_all=new_wall, old_route_ms_best=min(old_s) * 1e3,
                                      old_route_ms_all=[v * 1e3 for v in old_s], old_route_cuts_timed=baseline_cuts,
                                      speedup_wall=min(old_s) * 1e3 / min(new_wall), model_ms=model_ms, kernels_over_model=min(new_ms) / model_ms,
                                      longest_chain_cut=longest_cut, longest_chain=int(sizes_of[longest_cut].max()),
                                      longest_chain_cut_alone_ms_best=min(alone), longest_chain_cut_alone_ms_all=alone,
                                      max_abs_s_difference_to_old_route_cut0=float(np.nanmax(np.abs(s_new - s_old)))))
        entry["workgroup_sweep_rows_ms"] = {}                               # APD_SILHOUETTE_WORKGROUP: the same bits, another launch
        for wg in (256, 512, 1024):
            os.environ["APD_SILHOUETTE_WORKGROUP"] = str(wg)
            try:
                call(labels, 0)
                entry["workgroup_sweep_rows_ms"][str(wg)] = min(call(labels, 0)[0] for _ in range(3))
            finally:
                del os.environ["APD_SILHOUETTE_WORKGROUP"]
        out["sizes"][str(n)] = entry
        for b in per_cut + per_sample + [d_mat]:
            b.free()
        del d
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=list(SIZES))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-cuts", type=int, default=CUTS, help="cuts the old route is timed on per repeat (scaled to all 16)")
    ap.add_argument("--percentiles", type=float, nargs=2, default=(0.01, 0.5))
    args = ap.parse_args()
    print(json.dumps(measure(args.sizes, args.repeats, max(1, min(args.baseline_cuts, CUTS)), *args.percentiles)), flush=True)


if __name__ == "__main__":
    main()
