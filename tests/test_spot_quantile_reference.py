"""CPU tests of the spot score quantile checker (tests/_spot_quantile_reference.py): one example worked on paper, the dictated
construction the GPU tests rely on, and what the seeded cases must contain so that the GPU sweep cannot pass on empty ground."""
import numpy as np

import _spot_quantile_reference as qref
import _spot_reference as ref
from _path_reference import F, bits

INF = F(np.inf)


def test_worked_example():
    """Queries A (1 frame) and B (1 frame), both zeros; streams S (scores 3, 1, NaN, 1) and T (scores 0.5, +INF) by the dictated
    construction.  Pairs in the order (B, T), (A, S), (B, S), (A, S).
      by pair : four groups; (A, S): entries 4, 1 NaN, sorted 1 1 3; perc 0.5 -> k = 2 -> 3; perc 0.75 -> k = 3 = entries - nans: INDEX.
      by query: groups B = {(B, T), (B, S)} then A = {(A, S) twice}.  B: entries 6, sorted 0.5 1 1 3 INF, perc 0.5 -> k = 3 -> 3,
                perc 0.75 -> k = 4 -> +INF.  A: entries 8, 2 NaN, sorted 1 1 1 1 3 3; k = 4 -> 3; k = 6: INDEX.
      all     : entries 14, 3 NaN, sorted 0.5 1 1 1 1 1 1 3 3 3 INF; perc 0.5 -> k = 7 -> 3; perc 0.75 -> k = 10 -> +INF."""
    xa, s = qref.dictated([3.0, 1.0, np.nan, 1.0])
    xb, t = qref.dictated([0.5, np.inf])
    seqs = [xa, xb, s, t]
    pairs = [(1, 3), (0, 2), (1, 2), (0, 2)]
    curves = [ref.curves(seqs[x], seqs[y]) for x, y in pairs]
    lengths = [1] * 4
    assert np.array_equal(bits(ref.scores(*curves[1], 1)), bits(np.array([3.0, 1.0, np.nan, 1.0], dtype=F)))
    assert curves[1][1].tolist() == [1, 2, 3, 4]
    perc = [0.5, 0.75]
    v, st, group, entries, nans, ks = qref.quantiles(curves, lengths, pairs, "pair", perc)
    assert group.tolist() == [0, 1, 2, 3] and entries.tolist() == [2, 4, 4, 4] and nans.tolist() == [0, 1, 1, 1]
    assert ks == [[1, 1], [2, 3], [2, 3], [2, 3]]
    assert v[0].tolist() == [np.inf, np.inf] and v[1, 0] == 3.0 and st.tolist() == [[0, 0], [0, -7], [0, -7], [0, -7]]
    assert bits(v[1, 1:]).tolist() == [qref.NAN_BITS]
    v, st, group, entries, nans, ks = qref.quantiles(curves, lengths, pairs, "query", perc)
    assert group.tolist() == [0, 1, 0, 1] and entries.tolist() == [6, 8] and nans.tolist() == [1, 2] and ks == [[3, 4], [4, 6]]
    assert v[0].tolist() == [3.0, np.inf] and v[1, 0] == 3.0 and st.tolist() == [[0, 0], [0, -7]]
    v, st, group, entries, nans, ks = qref.quantiles(curves, lengths, pairs, "all", perc)
    assert group.tolist() == [0] * 4 and entries.tolist() == [14] and nans.tolist() == [3] and ks == [[7, 10]]
    assert v.tolist() == [[3.0, np.inf]] and st.tolist() == [[0, 0]]
    assert qref.quantiles([], [], [], "all", perc)[0].shape == (0, 2) and qref.groups_of([], "query") == ([], [])
    # -0.0 comes back as +0.0; the index is the f32 product, saturating
    assert bits(qref.sorted_scores(np.array([-0.0, 0.0, 1.0], dtype=F))[0]).tolist() == [0, 0, 0x3F800000]
    assert [qref.percentile_index(10, p) for p in (-1.0, np.nan, 0.0, 0.95, 1.0, 1e30)] == [0, 0, 0, 9, 10, 2 ** 64 - 1]
    assert qref.percentile_index(2 ** 24 + 3, 0.5) == 8388610 and (2 ** 24 + 3) // 2 == 8388609


def test_dictated_scores_come_back_bit_for_bit():
    """score(j) = s_j and start = j for the multisets the GPU tests dictate: 256 neighbours that share their top 24 key bits, many
    exponents, zeros, NaN and +INF."""
    near = (np.uint32(0x3F5A3C00) + np.arange(256, dtype=np.uint32)).view(F)
    wide = np.array([2.0 ** e for e in range(-40, 41, 3)] + [1.5 * 2.0 ** e for e in range(-39, 40, 5)], dtype=F)
    odd = np.array([0.0, np.nan, np.inf, 1.0, 0.1, 3.3333333, np.nan, 0.0, 7e-9, 12345.678], dtype=F)
    for scores in (near, wide, odd):
        x, y = qref.dictated(scores)
        cost, start = ref.curves(x, y)
        assert np.array_equal(bits(ref.scores(cost, start, 1)), bits(scores)) and start.tolist() == list(range(1, len(scores) + 1))
    assert len(set((bits(near) >> 8).tolist())) == 1 and len(set(bits(near).tolist())) == 256


def test_seeded_cases_hold_what_the_gpu_sweep_needs():
    cases = qref.seeded_cases()
    assert {c["by"] for c in cases} == set(qref.BYS) and {len(c["perc"]) for c in cases} == {1, 8}
    assert {c["seqs"][0].shape[1] for c in cases} == {8, 13}
    columns = 256
    lens = {(len(c["seqs"][x]), len(c["seqs"][y])) for c in cases for x, y in c["pairs"]}
    assert {n for n, _ in lens} >= {1, 7, 65}
    assert {m for _, m in lens} >= {1, 2, 63, 64, 65, columns - 1, columns, columns + 1, 2 * columns + 3}
    seen = set()
    for c in cases:
        pairs = c["pairs"]
        values, status, group, entries, nans, ks = qref.quantiles(c["curves"], c["lengths"], pairs, c["by"], c["perc"])
        pops, _ = qref.populations(c["curves"], c["lengths"], pairs, c["by"])
        if len(set(pairs)) < len(pairs):
            seen.add("repeated pair")
        if any(x == y for x, y in pairs):
            seen.add("x == y")
        if pairs != sorted(pairs):
            seen.add("shuffled")
        for g, pop in enumerate(pops):
            kept, n_nan = qref.sorted_scores(pop)
            assert n_nan == int(nans[g]) and len(pop) == int(entries[g])
            if n_nan:
                seen.add("nan")
            if np.any(kept == INF):
                seen.add("inf entry")
            if np.any(kept < 0):
                seen.add("negative")
            if c["by"] == "query" and len({len(c["seqs"][y]) for p, (_, y) in enumerate(pairs) if group[p] == g}) > 1:
                seen.add("query group of unequal streams")
            for q, k in enumerate(ks[g]):
                if k == len(kept):
                    assert status[g, q] == qref.ERR_INDEX and bits(values[g, q:q + 1])[0] == qref.NAN_BITS
                    seen.add("k == entries - nans" + (" with nans" if n_nan else ""))
                elif k == len(kept) - 1:
                    assert status[g, q] == qref.OK
                    seen.add("k == entries - nans - 1" + (" with nans" if n_nan else ""))
                elif k < len(kept):
                    if (k > 0 and kept[k - 1] == kept[k]) or (k + 1 < len(kept) and kept[k + 1] == kept[k]):
                        seen.add("tie across k")
                    if values[g, q] < 0:
                        seen.add("negative value")
                    if values[g, q] == INF:
                        seen.add("inf value")
    want = {"repeated pair", "x == y", "shuffled", "nan", "inf entry", "negative", "negative value", "query group of unequal streams",
            "k == entries - nans", "k == entries - nans with nans", "k == entries - nans - 1", "k == entries - nans - 1 with nans", "tie across k"}
    assert want <= seen, want - seen
