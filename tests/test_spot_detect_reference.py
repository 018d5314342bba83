"""CPU tests of the spot-detection checker (tests/_spot_detect_reference.py), no GPU: a hand-worked per-stream example, the
per-pair mode tied to what is already pinned (_spot_reference.hits and the host's apd_spot_hits), and the seeded case list of
tests/test_gpu_spot_detect.py, which must exercise the greedy in every case."""
import numpy as np

import _spot_detect_reference as det
import _spot_reference as ref

F = np.float32


def col(values):
    return np.array(values, dtype=F).reshape(-1, 1)


def test_hand_worked_per_stream_example():
    """Stream y = 5 1 2 5 1 3 5 2 4 3, templates A = 1 2 and B = 2 4 1, unit penalties, one feature (d = |x - y|).
    A: cost 7 1 0 3 1 1 4 1 3 3, start 1 2 2 2 5 5 5 8 8 10: column 3 ends the exact copy y[2..3] (score 0 / (2 + 2) = 0), column 6
       the window 5..6 = "1 3" (cost 1, score 1 / 4).
    B: cost 8 4 3 5 1 3 6 3 3 2, start 1 1 3 3 3 3 5 6 8 8: column 5 ends 3..5 = "2 5 1" (cost 1, score 1 / 6), column 10 ends 8..10 =
       "2 4 3" (cost 2, score 2 / 6).
    Thresholds 0.3 for A and 0.4 for B leave A the columns 3 and 6, B the columns 5 and 10.  One stream, so one group, in order:
    A@3 (0) accepted; B@5 (1/6) shares column 3 with it: rejected; A@6 (1/4) accepted; B@10 (1/3) accepted -- the loser's second-best
    window survives.  A third template, a copy of A listed last, ties with A in every candidate and loses each tie by pair index:
    its windows equal A's, which are accepted first."""
    y, a, b = col([5, 1, 2, 5, 1, 3, 5, 2, 4, 3]), col([1, 2]), col([2, 4, 1])
    cost_a, start_a = ref.curves(a, y)
    cost_b, start_b = ref.curves(b, y)
    assert cost_a.tolist() == [7, 1, 0, 3, 1, 1, 4, 1, 3, 3] and start_a.tolist() == [1, 2, 2, 2, 5, 5, 5, 8, 8, 10]
    assert cost_b.tolist() == [8, 4, 3, 5, 1, 3, 6, 3, 3, 2] and start_b.tolist() == [1, 1, 3, 3, 3, 3, 5, 6, 8, 8]
    seqs, pairs = [a, b, a.copy(), y], [(0, 3), (1, 3), (2, 3)]
    hits, off, labels, stats = det.detect(seqs, pairs, [0.3, 0.4, 0.3], per_stream=True)
    assert labels == [3] and off.tolist() == [0, 3]
    assert [(int(h["pair"]), int(h["end"]), int(h["start"]), float(h["cost"]), int(h["rank"])) for h in hits] == \
        [(0, 3, 2, 0.0, 0), (0, 6, 5, 1.0, 1), (1, 10, 8, 2.0, 2)]
    assert hits["score"].tolist() == [F(0.0), F(1.0) / F(4.0), F(2.0) / F(6.0)]
    assert stats == [{"candidates": 6, "hits": 3, "rejected": 3, "ties": 2, "pairs_hit": 2}]
    # each pair alone keeps its own best: B's window 3..5 is back, and the copy of A finds what A finds
    alone, off, labels, _ = det.detect(seqs, pairs, [0.3, 0.4, 0.3], per_stream=False)
    assert labels == [0, 1, 2] and off.tolist() == [0, 2, 4, 6]
    assert [(int(h["pair"]), int(h["end"]), int(h["start"]), int(h["rank"])) for h in alone] == \
        [(0, 3, 2, 0), (0, 6, 5, 1), (1, 5, 3, 0), (1, 10, 8, 1), (2, 3, 2, 0), (2, 6, 5, 1)]


def test_groups_follow_first_appearance_and_need_not_be_adjacent():
    pairs = [(0, 5), (1, 4), (2, 5), (0, 4), (0, 5), (3, 6)]
    assert det.groups_of(pairs, True) == ([0, 1, 0, 1, 0, 2], [5, 4, 6])
    assert det.groups_of(pairs, False) == (list(range(6)), list(range(6)))


def test_zero_signs_tie_and_nan_is_no_candidate():
    """-0.0 and +0.0 are one score: the smaller end decides, not the sign.  A NaN score or threshold gives no candidate."""
    cost = np.array([0.0, 3.0, -0.0, np.nan], dtype=F)
    start = np.array([1, 2, 3, 4], dtype=np.uint32)
    hits, off, _, _ = det.detect_curves([(cost, start)], [1], [(0, 1)], 1.0, False)
    assert [(int(h["end"]), int(h["start"])) for h in hits] == [(1, 1), (3, 3)] and off.tolist() == [0, 2]
    assert ref.bits(hits["score"]).tolist() == [0, 0x80000000]                # the record keeps the score's own bits
    none, off, _, _ = det.detect_curves([(cost, start)], [1], [(0, 1)], np.nan, False)
    assert len(none) == 0 and off.tolist() == [0, 0]


def test_per_pair_mode_is_the_pinned_picking(apd):
    """Record for record, bits of cost and score: the checker's per-pair mode, _spot_reference.hits and the host's apd_spot_hits."""
    from audio_pattern_discovery_amd.alignments import spot_hits
    rng = np.random.default_rng(11)
    for case in range(12):
        dim = int(rng.integers(1, 3))
        y = rng.integers(0, 3, (int(rng.integers(30, 90)), dim)).astype(F)
        xs = [rng.integers(0, 3, (int(rng.integers(1, 7)), dim)).astype(F) for _ in range(2)]
        pen = (1.0, 1.0, 1.0) if case % 3 else (1.0, 2.0, 0.5)
        curves = [ref.curves(x, y, *pen) for x in xs]
        thr = [det.median_threshold(curves[:1], [len(xs[0])]), F(np.inf)]
        hits, off, _, _ = det.detect_curves(curves, [len(x) for x in xs], [(0, 2), (1, 2)], thr, False)
        for p in range(2):
            mine = hits[int(off[p]):int(off[p + 1])]
            want = ref.hits(curves[p][0], curves[p][1], len(xs[p]), thr[p])
            host = spot_hits(curves[p][0], curves[p][1], len(xs[p]), thr[p])
            assert len(mine) == len(want) == len(host) and len(mine) >= 1
            assert np.all(mine["pair"] == p) and mine["rank"].tolist() == list(range(len(mine)))
            for other in (want, host):
                assert np.array_equal(mine["end"], other["end"]) and np.array_equal(mine["start"], other["start"])
                assert np.array_equal(ref.bits(mine["cost"]), ref.bits(other["cost"]))
                assert np.array_equal(ref.bits(mine["score"]), ref.bits(other["score"]))


def test_the_seeded_case_list_exercises_the_greedy():
    """Conditions on the cases tests/test_gpu_spot_detect.py runs, not measurements: in EVERY case some group has two hits or more,
    some candidate is rejected, and two different pairs tie exactly in (score, end)."""
    cases = det.seeded_cases()
    assert len(cases) == 40
    for seqs, pairs, thr, curves in cases:
        hits, off, labels, stats = det.detect_curves(curves, [len(seqs[x]) for x, _ in pairs], pairs, thr, True)
        assert labels == [3] and len(stats) == 1 and int(off[-1]) == len(hits)
        assert stats[0]["hits"] >= 2 and stats[0]["rejected"] >= 1 and stats[0]["ties"] >= 1, stats
        spans = sorted((int(h["start"]), int(h["end"])) for h in hits)
        assert all(a[1] < b[0] for a, b in zip(spans[:-1], spans[1:]))       # disjoint
