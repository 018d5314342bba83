"""The online detector's checker (tests/_spot_online_reference.py) against examples worked by hand, its properties, and the condition
the GPU test rests on: every seeded case shows every event of the machine.  No GPU.

Example 1, per pair.  One query of n = 2 frames, threshold 0.5, holdoff 2, origin 0.  score = cost / (n + end - start + 1).

    column  1     2     3      4      5     6     7      8     9      10
    start   1     1     2      3      3     3     6      8     8      9
    cost    3     1     0.5    0.5    5     1.5   1.5    0.75  0.5    1
    score   1     0.25  0.125  0.125  1     0.25  0.375  0.25  0.125  0.25

    2   candidate, nothing pending                          P = (end 2, start 1, 0.25)                         step 4
    3   start 2 <= P.end 2: overlap, 0.125 < 0.25           P = (3, 2, 0.125)                                  step 5, replaced
    4   start 3 <= P.end 3: overlap, 0.125 == 0.125         discarded, the earlier end stays                   step 5, equal
    5   no candidate; 5 - 3 = 2 is not > 2
    6   6 - 3 = 3 > 2: the timer emits (3, 2) rank 0, F = 3; then the candidate: start 3 <= F                  steps 1 and 3
    7   candidate, start 6 > F, nothing pending             P = (7, 6, 0.375)                                  step 4
    8   8 - 7 = 1: no timer; start 8 > P.end 7: disjoint    emits (7, 6) rank 1, F = 7, P = (8, 8, 0.25)       step 6
    9   start 8 <= 8: overlap, 0.125 < 0.25                 P = (9, 8, 0.125)                                  step 5, replaced
    10  start 9 <= 9: overlap, 0.25 > 0.125                 discarded                                          step 5
    the stream ends with (9, 8) pending: only a flush emits it, rank 2.

Example 2, per channel.  Two queries of 2 frames (pairs 0 and 1), thresholds 0.5, holdoff 1, origin 0.

    column        1    2      3      4    5      6
    pair 0 start  1    1      3      3    5      5
           cost   3    1      3      4    -0.0   0
           score  1    0.25   1      1    -0.0   0
    pair 1 start  1    2      2      4    4      6
           cost   3    0.75   0.5    3    0.0    3
           score  1    0.25   0.125  1    0.0    1

    2   both are candidates with 0.25: the tie goes to pair 0           P = (pair 0, end 2, start 1, 0.25)
    3   pair 1 alone: start 2 <= P.end 2, 0.125 < 0.25                  P = (pair 1, 3, 2, 0.125)
    4   no candidate; 4 - 3 = 1 is not > 1
    5   5 - 3 = 2 > 1: the timer emits (pair 1, 3, 2) rank 0, F = 3.  -0.0 and +0.0 tie: pair 0, its -0.0 kept   P = (pair 0, 5, 5, -0.0)
    6   pair 0 alone: start 5 <= P.end 5, 0 == -0.0: discarded
    a flush emits (pair 0, 5, 5) rank 1 with cost and score -0.0, the sign bit set."""
import numpy as np
import pytest

import _spot_online_cases as cases
import _spot_online_reference as online
from _path_reference import F, bits


def curve(cost, start):
    return np.array(cost, dtype=F), np.array(start, dtype=np.uint32)


EXAMPLE_1 = [curve([3, 1, 0.5, 0.5, 5, 1.5, 1.5, 0.75, 0.5, 1], [1, 1, 2, 3, 3, 3, 6, 8, 8, 9])]
EXAMPLE_2 = [curve([3, 1, 3, 4, -0.0, 0], [1, 1, 3, 3, 5, 5]), curve([3, 0.75, 0.5, 3, 0.0, 3], [1, 2, 2, 4, 4, 6])]


def rows(hits):
    return [(int(h["pair"]), int(h["end"]), int(h["start"]), float(h["cost"]), float(h["score"]), int(h["rank"])) for h in hits]


def test_per_pair_example_worked_by_hand():
    stats = online.new_stats()
    hits, when = online.channel_hits(0, EXAMPLE_1, [2], [0.5], False, 2, stats=stats)
    assert rows(hits) == [(0, 3, 2, 0.5, 0.125, 0), (0, 7, 6, 1.5, 0.375, 1)] and when.tolist() == [6, 8]
    assert {e: stats[e] for e in online.EVENTS} == {"replace": 2, "equal_discard": 1, "floor_discard": 1, "timer": 1, "displace": 1, "tie": 0}
    hits, when = online.channel_hits(0, EXAMPLE_1, [2], [0.5], False, 2, flush_at=[10])
    assert rows(hits)[2] == (0, 9, 8, 0.5, 0.125, 2) and when.tolist() == [6, 8, 10]
    # the timer edge: pushed up to P.end + holdoff = 5 nothing is out, one column more and the hit is
    assert len(online.channel_hits(0, EXAMPLE_1, [2], [0.5], False, 2, upto=5)[0]) == 0
    assert rows(online.channel_hits(0, EXAMPLE_1, [2], [0.5], False, 2, upto=6)[0]) == [(0, 3, 2, 0.5, 0.125, 0)]
    # the threshold is strict: at exactly 0.125 nothing is a candidate; armed at column 3, the window (3, 2) starts before the origin
    assert len(online.channel_hits(0, EXAMPLE_1, [2], [0.125], False, 2, flush_at=[10])[0]) == 0
    assert rows(online.channel_hits(0, EXAMPLE_1, [2], [0.5], False, 2, origin=3)[0]) == [(0, 7, 6, 1.5, 0.375, 0)]
    # the timer never fires: displacement and flush only
    hits, when = online.channel_hits(0, EXAMPLE_1, [2], [0.5], False, online.NEVER, flush_at=[10])
    assert [r[1:3] for r in rows(hits)] == [(3, 2), (7, 6), (9, 8)] and when.tolist() == [7, 8, 10]


def test_per_channel_example_worked_by_hand():
    stats = online.new_stats()
    hits, when = online.channel_hits(0, EXAMPLE_2, [2, 2], [0.5, 0.5], True, 1, flush_at=[6], stats=stats)
    assert rows(hits) == [(1, 3, 2, 0.5, 0.125, 0), (0, 5, 5, 0.0, 0.0, 1)] and when.tolist() == [5, 6]
    assert bits(hits["cost"])[1] == 0x80000000 and bits(hits["score"])[1] == 0x80000000          # the zero keeps its sign
    assert stats["tie"] == 2 and stats["replace"] == 1 and stats["equal_discard"] == 1 and stats["timer"] == 1
    # per pair the same curves are two machines: pair 0's (2, 1) is nobody's overlap and leaves by the timer at column 4
    alone, _ = online.channel_hits(0, EXAMPLE_2, [2, 2], [0.5, 0.5], False, 1, flush_at=[6])
    assert [r[:3] + r[5:] for r in rows(alone)] == [(0, 2, 1, 0), (0, 5, 5, 1), (1, 3, 2, 0), (1, 5, 4, 1)]
    # as channel 3 of a session the pairs are 6 and 7, the group 3
    shifted, _ = online.channel_hits(3, EXAMPLE_2, [2, 2], [0.5, 0.5], True, 1, flush_at=[6])
    assert shifted["pair"].tolist() == [7, 6] and online.group_of(shifted, 2, True).tolist() == [3, 3]


def test_reset_drops_pending_windows_and_keeps_ranks():
    # example 1 up to column 9, where (9, 8) is pending; then a fresh table at first_column 100 whose curves are example 1's again
    after = [curve(EXAMPLE_1[0][0], EXAMPLE_1[0][1] + 100)]
    hits, when = online.with_reset(0, EXAMPLE_1, after, 9, 100, [2], [0.5], False, 2)
    assert [r[1:3] + r[5:] for r in rows(hits)] == [(3, 2, 0), (7, 6, 1), (103, 102, 2), (107, 106, 3)]
    assert when.tolist() == [6, 8, 106, 108]


@pytest.fixture(scope="module", params=sorted(cases.SPECS))
def seeded(request):
    c = cases.case(request.param)
    stats = online.new_stats()
    parts = [online.channel_hits(k, c["curves"][k], c["lengths"], c["thresholds"][k], c["per_stream"], c["holdoff"], stats=stats)
             for k in range(len(c["streams"]))]
    return c, parts, stats


def test_every_seeded_case_shows_every_event(seeded):
    """The condition the GPU test rests on: it cannot pass without a replacement, a discard at equal scores, a discard by the
    floor, an emission by the timer, one by displacement and -- per channel -- two pairs tying at one column."""
    c, _, stats = seeded
    for event in online.EVENTS:
        if event == "tie" and not c["per_stream"]:
            continue
        assert stats[event] >= 1, (event, stats)
    assert len(set(c["thresholds"].ravel().tolist())) > 1                    # per-pair thresholds that differ


def test_properties_of_the_emitted_hits(seeded):
    c, parts, _ = seeded
    n_q = len(c["queries"])
    for k, (hits, when) in enumerate(parts):
        assert len(hits) >= 3
        groups = online.group_of(hits, n_q, c["per_stream"])
        for g in np.unique(groups):
            mine, emitted = hits[groups == g], when[groups == g]
            assert mine["rank"].tolist() == list(range(len(mine)))
            assert np.all(mine["start"] <= mine["end"]) and np.all(mine["start"][1:] > mine["end"][:-1])     # disjoint, ends ascending
            assert np.all(emitted > mine["end"]) and np.all(emitted <= mine["end"].astype(np.int64) + c["holdoff"] + 1)
        for h in hits:                                                       # every hit is a candidate, with the curve's bits
            q = int(h["pair"]) - k * n_q
            cost, start = c["curves"][k][q]
            j = int(h["end"])
            assert int(start[j - 1]) == int(h["start"]) != 0 and bits(cost[j - 1]) == bits(h["cost"])
            score = online.score_at(cost[j - 1], start[j - 1], c["lengths"][q], j)
            assert bits(score) == bits(h["score"]) and score < c["thresholds"][k, q]


def test_emission_does_not_depend_on_how_upto_steps(seeded):
    """Running to column L in one go gives what has been emitted by column L of the whole run: a prefix per group, decided by the
    columns up to L alone."""
    c, parts, _ = seeded
    n_q = len(c["queries"])
    for k, (hits, when) in enumerate(parts):
        m = len(c["streams"][k])
        groups = online.group_of(hits, n_q, c["per_stream"])
        for L in list(range(0, m + 1, 7)) + [m]:
            got, got_when = online.channel_hits(k, c["curves"][k], c["lengths"], c["thresholds"][k], c["per_stream"], c["holdoff"], upto=L)
            keep = when <= L
            assert online.same_hits(got, hits[keep]) and np.array_equal(got_when, when[keep]), (k, L)
            assert np.array_equal(online.group_of(got, n_q, c["per_stream"]), groups[keep])


def test_the_special_conditions_of_the_gpu_cases_hold():
    """What tests/test_gpu_spot_online.py relies on beyond the events: a column where a -0.0 and a +0.0 candidate tie, and pushes of
    64 columns that carry a pending window across a boundary and see it replaced by a candidate behind it."""
    assert cases.zero_sign_ties(cases.case("zeros_d2")) >= 1
    for name in ("channels_d5", "channels_d13"):
        carried, replaced = cases.carried_across(cases.case(name), 64)
        assert carried >= 1 and replaced >= 1, name
    assert cases.carried_across(cases.case("pairs_d13"), 64)[0] >= 1
