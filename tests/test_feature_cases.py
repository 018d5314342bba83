"""CPU tests of tests/_feature_cases.py, the generator of tests/test_gpu_feature_sweep.py: the draws are deterministic, stay inside the
budget of checker cells, cover over the committed seeds what the sweep exists for, and the two restatements of the streaming contract
(the ring session, chunk by chunk; the whole-stream table through expected()) agree on every window a scenario asks.  No GPU and no
product code: everything here is asserted on the drawn cases."""
import numpy as np
import pytest

import _feature_cases as fc
import _kernel_table as kt
import _spot_path_reference as spref

FEATURE = [(seed, k) for seed in fc.FEATURE_SEEDS for k in range(fc.FEATURE_CASES_PER_SEED)]
STREAM = [(seed, k) for seed in fc.STREAM_SEEDS for k in range(fc.STREAM_CASES_PER_SEED)]


def test_the_committed_lists():
    assert len(fc.FEATURE_SEEDS) == len(fc.STREAM_SEEDS) == 3 and fc.FEATURE_CASES_PER_SEED == 12 and fc.STREAM_CASES_PER_SEED == 4
    assert fc.BAND_PCTS == fc.fuzz_band_list()
    assert fc.CASE_BUDGET == 250_000 and fc.SEED_BUDGET == 2_000_000


def test_draws_are_deterministic():
    for seed, k in FEATURE[:6] + FEATURE[-3:]:
        a = fc.feature_case(seed, k)
        fc._FEATURE.clear()
        b = fc.feature_case(seed, k)
        assert a is not b and fc.case_bytes(a) == fc.case_bytes(b) and a.ops == b.ops and a.caps == b.caps
        assert (a.dim, a.pens, a.pct, a.form, a.poison, a.lengths, a.n_first) == (b.dim, b.pens, b.pct, b.form, b.poison, b.lengths, b.n_first)
    for seed, k in STREAM[:3]:
        a = fc.stream_case(seed, k)
        fc._STREAM.clear()
        b = fc.stream_case(seed, k)
        assert a is not b and fc.stream_bytes(a) == fc.stream_bytes(b)
        assert [fc.describe(x) for x in a.actions] == [fc.describe(x) for x in b.actions] and a.sessions == b.sessions


def test_every_case_and_every_seed_stays_inside_the_budget():
    for seeds, count, make in ((fc.FEATURE_SEEDS, fc.FEATURE_CASES_PER_SEED, fc.feature_case),
                               (fc.STREAM_SEEDS, fc.STREAM_CASES_PER_SEED, fc.stream_case)):
        for seed in seeds:
            cells = [make(seed, k).cells for k in range(count)]
            print(make.__name__, seed, cells)
            assert max(cells) <= fc.CASE_BUDGET and sum(cells) <= fc.SEED_BUDGET, (seed, cells)


def test_the_cell_count_is_the_checkers_own():
    """feature_cells against a count taken inside the checker, on one drawn case: the banded tables of its paths."""
    import _path_reference as pref
    case, op = next((c, o) for c in (fc.feature_case(*sk) for sk in FEATURE) for o in c.ops if o["op"] == "paths")
    x, y = min(op["pairs"], key=lambda p: case.lengths[p[0]] * case.lengths[p[1]])
    n, m = case.lengths[x], case.lengths[y]
    sparse, _ = pref.table(case.seqs[x], case.seqs[y], pref.band_from_pct(case.pct, max(n, m)))
    assert fc.band_cells(n, m, case.pct) == len(sparse) - 1


def test_the_feature_cases_cover_what_the_sweep_is_for():
    cases = [fc.feature_case(seed, k) for seed, k in FEATURE]
    rows = kt.parse_spot_register_rows()
    classes, widest, wide_path, fed = set(), 0, 0, 0
    for c in cases:
        assert 8 <= len(c.seqs) <= 16 and all(1 <= c.lengths[s] <= 120 for s in c.streams)
        assert [len(s) for s in c.seqs] == c.lengths and all(s.shape[1] == c.dim and s.dtype == np.float32 for s in c.seqs)
        for op in c.ops:
            if op["op"] == "spot":
                here = {fc.spot_class(c.dim, c.lengths[x])[0] if fc.resident_dim(c.dim) else -1 for x, _ in op["pairs"]}
                rows_here = {kt.spot_rows_per_lane(c.lengths[x]) for x, _ in op["pairs"]}
                classes |= here - {-1}
                widest = max(widest, len({min(r, rows + 1) for r in rows_here}))
            if op["op"] == "paths":
                wide_path += sum(2 * fc.path_half_width(c.lengths[x], c.lengths[y], c.pct) + 1 > 128 for x, y in op["pairs"])
            if op["op"] == "barycenters":
                fed += op["on_device"] and any(op["sets"])
            if op["op"] in ("cross", "cross_linkage"):
                assert c.form.startswith("joined")
    assert classes == set(range(rows + 1)), classes
    assert widest >= 3 and wide_path >= 1 and fed >= 1
    assert {c.dim_kind for c in cases} == {"kernel", "padded", "beyond"}
    assert {c.form for c in cases} == {"plain", "joined-AB", "joined-BA", "refilled"}
    for name in ("APD_PATH_WORKSPACE_BYTES", "APD_SPOT_WORKSPACE_BYTES"):
        assert {c.caps[name][0] for c in cases} == {"unset", "one", "chunks"}, name
    assert {c.pen_kind for c in cases} == {"unit", "equal", "drawn"}
    assert sum(c.poison is not None for c in cases) >= 2
    copies = [c for c in cases if c.copy is not None]
    assert len(copies) >= 3 and all(c.lengths[c.copy[0]] == c.lengths[c.copy[1]] for c in copies)
    assert all(np.array_equal(c.seqs[c.copy[0]], c.seqs[c.copy[1]]) for c in copies if c.poison is None)      # a poison comes after the copy
    assert {op["op"] for c in cases for op in c.ops} == set(fc.OPERATIONS)
    # a joined batch whose second set is the longer one on average is resident in swapped order
    swapped = {sum(c.lengths[:c.n_first]) * (len(c.lengths) - c.n_first) < sum(c.lengths[c.n_first:]) * c.n_first
               for c in cases if c.form.startswith("joined")}
    assert swapped == {True, False}


def test_a_drawn_cap_cuts_its_list_into_two_to_four_chunks():
    seen = 0
    for seed, k in FEATURE:
        c = fc.feature_case(seed, k)
        kind, value = c.caps["APD_PATH_WORKSPACE_BYTES"]
        if kind == "chunks":
            op = next(o for o in c.ops if o["op"] == "paths")
            assert 2 <= fc._chunks([np.array(v) for v in fc.path_cap_costs(c.lengths, op["pairs"], c.pct)], value) <= 4
            seen += 1
        kind, value = c.caps["APD_SPOT_WORKSPACE_BYTES"]
        if kind == "chunks":
            op = next(o for o in c.ops if o["op"] == "spot" and o["curves"])
            assert 2 <= fc._chunks([np.array([8 * c.lengths[y]]) for _, y in op["pairs"]], value) <= 4
            seen += 1
    assert seen >= 2


def test_the_stream_scenarios_cover_the_state_machine():
    wraps = keep_mid = long_push = infinite = 0
    outcomes = set()
    for seed, k in STREAM:
        c = fc.stream_case(seed, k)
        assert 2 <= len(c.templates) <= 4 and 1 in c.lengths and len(c.sessions) == 2 and 12 <= len(c.actions) <= 25
        assert c.sessions[0]["queries"] != c.sessions[1]["queries"] or c.sessions[0]["channels"] != c.sessions[1]["channels"]
        origin = [[0] * s["channels"] for s in c.sessions]
        first = [[0] * s["channels"] for s in c.sessions]
        pushed = [[0] * s["channels"] for s in c.sessions]
        H = [s["history"] for s in c.sessions]
        for act in c.actions:
            s, want = act["session"], act["want"]
            channels = range(c.sessions[s]["channels"])
            if act["kind"] == "push":
                assert all(size in fc.PUSH_SIZES for size in act["sizes"])
                for ch in channels:
                    pushed[s][ch] += act["sizes"][ch]
                    assert pushed[s][ch] <= fc.CHANNEL_COLUMNS
                    wraps += H[s] > 0 and want["columns"][ch] - origin[s][ch] >= 3 * H[s]
                long_push += H[s] > 0 and max(act["sizes"]) > H[s]
                if act["infinite"]:                                 # the first frame behind a reset of pushed data, curves returned
                    assert act["curves"] and all(np.isinf(chunk[0]).any() for chunk in act["chunks"] if len(chunk))
                    infinite += max(c.sessions[s]["lens"]) >= 2 and any(0 < v < 1 << 31 for v in want["columns"])
            elif act["kind"] == "reset":
                for ch in channels if act["channel"] is None else [act["channel"]]:
                    first[s][ch] = origin[s][ch] = act["first_column"]
            elif act["kind"] == "keep":
                keep_mid += any(want["columns"][ch] > first[s][ch] for ch in channels)
                H[s] = act["history"]
                origin[s] = list(want["columns"])
            elif act["kind"] == "paths":
                outcomes |= set(want["outcomes"])
            assert want["H"] == H[s]
    assert wraps >= 1 and keep_mid >= 1 and long_push >= 1 and infinite >= 2
    assert outcomes == set(fc.OUTCOMES), set(fc.OUTCOMES) - outcomes


def test_a_single_channel_is_reset_after_data():
    """A reset of ONE channel of a session with several, after that channel has been pushed to."""
    found = 0
    for seed, k in STREAM:
        c = fc.stream_case(seed, k)
        data = [[0] * s["channels"] for s in c.sessions]
        for act in c.actions:
            s = act["session"]
            if act["kind"] == "push":
                data[s] = [d + size for d, size in zip(data[s], act["sizes"])]
            elif act["kind"] == "reset" and act["channel"] is not None and c.sessions[s]["channels"] > 1:
                found += data[s][act["channel"]] > 0
    assert found >= 1


@pytest.mark.parametrize("seed", fc.STREAM_SEEDS)
def test_the_two_stream_checkers_agree_on_every_scenario(seed):
    """The ring session (what the GPU is compared with) against _spot_path_reference.answer on the whole stream since the reset,
    passed through expected(): every window of every `paths` action."""
    asked = 0
    for k in range(fc.STREAM_CASES_PER_SEED):
        c = fc.stream_case(seed, k)
        for a, act in enumerate(c.actions):
            if act["kind"] != "paths":
                continue
            for t, w in enumerate(act["windows"]):
                ring, whole = act["want"]["answers"][t], fc.whole_answer(c, act, t)
                assert spref.same_steps(ring[0], whole[0]) and int(ring[1]) == int(whole[1]), (seed, k, a, w)
                assert spref.bits([ring[2]])[0] == spref.bits([whole[2]])[0], (seed, k, a, w)
                asked += 1
    assert asked >= 10


def test_the_predicted_kernels_are_instantiations_of_the_header():
    want = set(kt.spot_kernels())
    feature = set().union(*(fc.feature_triples(fc.feature_case(seed, k)) for seed, k in FEATURE))
    stream = set().union(*(fc.stream_triples(fc.stream_case(seed, k)) for seed, k in STREAM))
    assert {t[0] for t in feature} == {"sweep", "record"} and {t[0] for t in stream} == {"stream", "streamrec"}
    assert all(t[1:] in want for t in feature | stream)
    assert len(feature) >= 8 and len(stream) >= 6
