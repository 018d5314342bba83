#!/usr/bin/env python3
"""Cross alignment against all-pairs alignment at the same number of pairs, on the cfg-3 shape (length ~1024, D = 13, band 6.25 %,
synth.make_sequences), in one process:

  (a) apd_align_cross of 256 x 4096 sequences: 1 048 576 unordered pairs;
  (b) apd_align_all on a 1449-sequence batch of the same generator: 1 049 076 unordered pairs, twice (the run-to-run spread).

Both legs are warmed once and timed with the library's own events (apd_last_kernel_ms).  Prints ONE JSON line: the times, the
reference-loop cell updates per second of each leg (cells from oracle.dtw_cells, both ordered pairs of every unordered one) and
the ratio cross / all-pairs of those rates.  APD_DEBUG_PLAN=1 in the environment also prints the tile
classes of both plans on stderr.

    python tools/cross_bench.py
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_FIRST, N_SECOND, N_ALL, LENGTH, DIM, PCT = 256, 4096, 1449, 1024, 13, 0.0625


def ordered_cells(lens_x, lens_y, oracle, all_pairs):
    """Cells the reference's loops visit for every ordered pair (x, y) and (y, x), x from lens_x, y from lens_y (all_pairs: x != y of
    one set), summed per distinct pair of lengths."""
    ux, cx = np.unique(lens_x, return_counts=True)
    uy, cy = np.unique(lens_y, return_counts=True)
    total = 0
    for n, kn in zip(ux, cx):
        for m, km in zip(uy, cy):
            pairs = int(kn) * int(km) - (int(kn) if all_pairs and n == m else 0)     # ordered pairs (x, y) with these lengths
            if pairs:
                band = oracle.warping_band(PCT, max(int(n), int(m)))
                total += pairs * (oracle.dtw_cells(int(n), int(m), band) if all_pairs else
                                  oracle.dtw_cells(int(n), int(m), band) + oracle.dtw_cells(int(m), int(n), band))
    return total


def main():
    from audio_pattern_discovery_amd import _lib, synth
    from audio_pattern_discovery_amd.alignments import Batch
    from audio_pattern_discovery_amd.discovery import Discovery
    from oracle import binding as oracle
    oracle.build()

    ctx = _lib.Context(0)
    ctx.set_timing(True)
    cfg = Discovery(warping_band_percentage=PCT).align_config()
    L = _lib.lib()
    out = dict(shape=dict(length=LENGTH, dim=DIM, band_pct=PCT))

    # (a) cross: one corpus of the generator, cut into the two sets
    frames, offsets = synth.make_sequences(N_FIRST + N_SECOND, LENGTH, DIM, seed=0xC205)
    seqs = synth.split(frames, offsets)
    lens = np.diff(offsets.astype(np.int64))

    def batch(part):
        off = np.zeros(len(part) + 1, np.uint64)
        off[1:] = np.cumsum([len(s) for s in part])
        return Batch(ctx, np.concatenate(part, axis=0), off, DIM)

    first, second = batch(seqs[:N_FIRST]), batch(seqs[N_FIRST:])
    joined = Batch.join(first, second)
    d_fs, d_sf = ctx.alloc(4 * N_FIRST * N_SECOND), ctx.alloc(4 * N_FIRST * N_SECOND)
    cross_ms = []
    for _ in range(3):                                              # the first run warms (plan, code objects)
        _lib.check(L.apd_align_cross_device_async(ctx.handle, joined.handle, C.byref(cfg), d_fs.at(), d_sf.at()), ctx.handle)
        ctx.synchronize()
        cross_ms.append(ctx.last_kernel_ms())
    la, lb = lens[:N_FIRST], lens[N_FIRST:]
    # the kernels sweep the sequence of the SECOND resident segment as rows; the first segment is the set with the larger mean length
    seg0, seg1 = (lb, la) if la.sum() * len(lb) < lb.sum() * len(la) else (la, lb)
    cross_cells = ordered_cells(la, lb, oracle, False)
    out["cross"] = dict(n_first=N_FIRST, n_second=N_SECOND, unordered_pairs=N_FIRST * N_SECOND, kernel_ms=cross_ms[1:], cells=cross_cells,
                        cell_updates_per_s=cross_cells / (min(cross_ms[1:]) * 1e-3),
                        rows_longer_share=float((seg1[None, :] > seg0[:, None]).mean()))
    for b in (d_fs, d_sf):
        b.free()
    for b in (joined, second, first):
        b.close()

    # (b) all pairs of a batch with as many unordered pairs
    frames, offsets = synth.make_sequences(N_ALL, LENGTH, DIM, seed=0xC206)
    lens = np.diff(offsets.astype(np.int64))
    whole = Batch(ctx, frames, offsets, DIM)
    d_out = ctx.alloc(4 * N_ALL * N_ALL)
    all_ms = []
    for _ in range(3):
        _lib.check(L.apd_align_all_device_async(ctx.handle, whole.handle, C.byref(cfg), d_out.at()), ctx.handle)
        ctx.synchronize()
        all_ms.append(ctx.last_kernel_ms())
    all_cells = ordered_cells(lens, lens, oracle, True)
    out["all_pairs"] = dict(n_seq=N_ALL, unordered_pairs=N_ALL * (N_ALL - 1) // 2, kernel_ms=all_ms[1:], cells=all_cells,
                            cell_updates_per_s=all_cells / (min(all_ms[1:]) * 1e-3))
    out["rate_ratio_cross_over_all_pairs"] = out["cross"]["cell_updates_per_s"] / out["all_pairs"]["cell_updates_per_s"]
    d_out.free()
    whole.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
