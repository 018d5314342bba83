#!/usr/bin/env python3
"""Macro-steps per workgroup of the systolic DTW kernels for a bench workload, counted on its seeded lengths without a GPU.
usage: tools/sweep_steps_model.py [workload] [C]      (default cfg3, C = 9)

The model is the shared-column kernel's: 16 x 16 tiles in resident order (longest first), 4 x 4 sub-blocks, the workgroup's
largest bound, rounded up to the unroll U (csrc/dtw_systolic.h).  Three bounds per pair with rows n, columns m, half-width w:
  all lanes through the last row   (n - 1) + ceil((2w + 1) / C)        rows = a, the longer sequence   (before)
  stop at the capture              (n - 1) + (m - n + w) // C + 1      rows = a
  rows = the shorter sequence      the same with rows = b               (sweep_steps_needed, csrc/apd_internal.h)
Only the lengths matter, and make_sequences draws them first from its seed, so no frames are generated."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (WORKLOADS and the seed rule of its inputs)


def lengths(name):
    wl = bench.WORKLOADS[name]
    rng = np.random.default_rng(0xA9D0 + sum(map(ord, name)) % 97)       # bench.py's seed for synth.make_sequences
    jitter = wl.get("jitter")
    jitter = max(wl["length"] // 32, 0) if jitter is None else jitter
    lens = rng.integers(max(wl["length"] - jitter, 1), wl["length"] + jitter + 1, size=wl["n_seq"])
    return np.sort(lens)[::-1].astype(np.int64), np.float32(wl["pct"])


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "cfg3"
    C = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    U = C + 1 if (C + 1) % 2 == 0 else 2 * (C + 1)
    lens, pct = lengths(name)
    n_seq = len(lens)
    tiles = (n_seq + 15) // 16
    lens = np.concatenate([lens, np.zeros(tiles * 16 - n_seq, np.int64)])
    total = {"all lanes through the last row": 0, "stop at the capture": 0, "plus rows = the shorter sequence": 0}
    groups = 0
    for ta in range(tiles):
        n = lens[ta * 16:(ta + 1) * 16][:, None] + np.zeros((1, 16), np.int64)
        ia = np.arange(ta * 16, (ta + 1) * 16)[:, None]
        for tb in range(ta, tiles):
            m = lens[tb * 16:(tb + 1) * 16][None, :] + np.zeros((16, 1), np.int64)
            ib = np.arange(tb * 16, (tb + 1) * 16)[None, :]
            swept = (ia < ib) & (ib < n_seq) & (n >= 2) & (m >= 2)
            mx = np.maximum(n, m)
            band = np.minimum((pct * mx.astype(np.float32)).astype(np.int64), mx)
            w = np.maximum(band, np.abs(n - m)) + 2
            bounds = ((n - 1) + (2 * w + 1 + C - 1) // C, (n - 1) + (m - n + w) // C + 1, (m - 1) + (n - m + w) // C + 1)
            for key, steps in zip(total, bounds):
                wg = np.where(swept, steps, 0).reshape(4, 4, 4, 4).max(axis=(1, 3))
                total[key] += int(((wg + U - 1) // U * U).sum())
            groups += int((swept.reshape(4, 4, 4, 4).max(axis=(1, 3))).sum())
    base = total["all lanes through the last row"]
    print("%s: %d sequences, C = %d, U = %d, %d sweeping workgroups" % (name, n_seq, C, U, groups))
    for key, v in total.items():
        print("%-34s %8.1f macro-steps per workgroup   ratio %.3f" % (key, v / groups, v / base))


if __name__ == "__main__":
    main()
