"""CPU tests of the checker tests/_spot_stream_path_reference.py: a session that keeps only H columns in rings answers every window
that lies inside them exactly as tests/_spot_path_reference.py answers it on the whole stream (steps, found start and score, bit
for bit, shifted by first_column), says "aged out" exactly where the contract of include/apd.h says so, and its curves and bests stay
those of tests/_spot_stream_reference.py -- for H below, at and above a wavefront and the chunk sizes, under the chunkings of
tests/test_gpu_spot_stream.py (a push longer than H, pushes of one column, zero-length chunks)."""
import numpy as np
import pytest

import _spot_path_reference as ref
import _spot_stream_path_reference as hist
import _spot_stream_reference as sref
from test_gpu_spot_stream import CHUNKINGS

F = np.float32
SKEWED = (1.0, 2.0, 0.5)
HISTORIES = (1, 24, 50, 64, 128)
QUERY_OF = {40: 13, 91: 30}                    # frames of the query per stream length


def case(m):
    rng = np.random.default_rng(1000 + m)
    return rng.integers(0, 3, (QUERY_OF[m], 2)).astype(F), rng.integers(0, 3, (m, 2)).astype(F)   # small integers: full of exact ties


_TABLES = {}


def table(m):
    if m not in _TABLES:
        x, y = case(m)
        _TABLES[m] = ref.table(x, y, *SKEWED)
    return _TABLES[m]


def same(got, want):
    return ref.same_steps(got[0], want[0]) and int(got[1]) == int(want[1]) and ref.bits([got[2]])[0] == ref.bits([want[2]])[0]


@pytest.mark.parametrize("first_column", (0, 1000003))
@pytest.mark.parametrize("history", HISTORIES)
@pytest.mark.parametrize("m", (40, 91))
def test_ring_session_equals_the_whole_table_and_ages_out_by_the_contract(m, history, first_column):
    x, y = case(m)
    n, tab = len(x), table(m)
    traced = aged = 0
    for sizes in CHUNKINGS[m]:
        session = hist.Session(x, *SKEWED, first_column=first_column, history=history)
        plain = sref.Session(x, *SKEWED, first_column=first_column)
        for chunk in sref.split(y, sizes):
            got, want = session.push(chunk), plain.push(chunk)
            assert np.array_equal(ref.bits(got[0]), ref.bits(want[0])) and np.array_equal(got[1], want[1])
            assert np.array_equal(got[2].reshape(1).view(np.uint32), want[2].reshape(1).view(np.uint32))
            first, last = session.kept()
            assert (first, last) == (max(first_column + 1, last - history + 1), first_column + plain.column - first_column)
            for end in range(max(first_column + 1, last - history - 2), last + 1):
                s_rel = tab[1][n][end - first_column]
                for start in {s_rel + first_column if s_rel else 0, end}:          # the table's start, and (mostly) a wrong one
                    rel = ref.answer(tab, n, end - first_column, start - first_column if start else 0)
                    want_w = hist.expected(rel, n, first_column, (first, last), end, start)
                    assert same(session.answer(end, start), want_w), (sizes, end, start)
                    if start == s_rel + first_column and start:
                        traced += len(want_w[0]) > 0
                        aged += len(want_w[0]) == 0
            assert same(session.answer(0, 0), hist.NONE)
    assert (traced >= 10 or history == 1) and (aged >= 10 or history >= m)       # H = 1 traces one-column windows only: rare here


def test_keep_in_mid_stream_starts_empty_and_reset_empties():
    x, y = case(40)
    n, tab = len(x), table(40)
    session = hist.Session(x, *SKEWED)
    session.push(y[:10])
    assert session.kept() == (11, 10)
    session.keep(8)
    assert session.kept() == (11, 10)                                              # empty behind the current column
    session.push(y[10:15])
    assert session.kept() == (11, 15)
    session.push(y[15:30])
    assert session.kept() == (23, 30)
    for end in range(23, 31):
        start = tab[1][n][end]
        assert same(session.answer(end, start), hist.expected(ref.answer(tab, n, end, start), n, 0, (23, 30), end, start))
    session.keep(3)
    assert session.kept() == (31, 30)
    session.reset(7)
    assert session.kept() == (8, 7)


def test_hand_case():
    """include/apd.h: x = [0, 1], y = [0, 1, 0], end 3: start 2, cost 2.0 -- traced with H = 2, aged out one column later."""
    x, y = np.array([[0], [1]], dtype=F), np.array([[0], [1], [0]], dtype=F)
    session = hist.Session(x, history=2)
    for k in range(3):
        session.push(y[k:k + 1])
    steps, found, score = session.answer(3, 2)
    assert found == 2 and steps["cost"][-1] == 2.0 and [tuple(int(v) for v in (s["i"], s["j"], s["op"])) for s in steps][-1][:2] == (2, 3)
    session.push(y[:1])
    steps, found, score = session.answer(3, 2)
    assert len(steps) == 0 and found == 2 and score == F(2.0) / F(4.0)
