"""The inputs of tests/test_gpu_feature_sweep.py and tools/debug/fuzz_features.py, drawn and not chosen by hand: TEST INFRASTRUCTURE,
no GPU, no product code.

feature_case(seed, k): one corpus -- a frame dimension, 8 .. 16 sequences in two sets (queries of every spot row class, streams of
1 .. 120 frames), Gaussian / small-integer / random-walk values, now and then an exact copy or a poisoned sequence, penalties, a band
percentage, a batch form and two workspace caps -- and a shuffled list of operations on it (paths, spot, spot_hits, spot_paths,
cross, cross_linkage, align_all, medoids, barycenters).  stream_case(seed, k): one streaming scenario -- templates, two live sessions
and 12 .. 25 actions (push -- now and then with an infinite first frame behind a reset --, reset, keep, paths, columns, history) addressed to either, with what the chunk-by-chunk model
(tests/_spot_stream_path_reference.py::Session, one per (query, channel)) says of every action recorded beside it; the windows
asked of `paths` come from that model.  Both are deterministic in (seed, k), and both count the checker DP cells the case costs and
redraw the LENGTHS (never the operations) until the count fits the budget.  What a case is predicted to dispatch -- the (kind, RT, D)
of the spotting kernels -- is computed here from lengths and dimensions alone (tests/_kernel_table.py)."""
import re
import os
import types
import zlib

import numpy as np

import _kernel_table as kt
import _path_reference as pref
import _spot_path_reference as spref
import _spot_reference as sref
import _spot_stream_path_reference as hist

F = np.float32
FEATURE_SEEDS = (101, 102, 103)
STREAM_SEEDS = (201, 202, 203)
FEATURE_CASES_PER_SEED = 12
STREAM_CASES_PER_SEED = 4
CASE_BUDGET = 250_000                           # checker DP cells of one case (about 2 us each)
SEED_BUDGET = 2_000_000                         # of one seed: one GPU test function
BAND_PCTS = (0.0, 0.01, 0.0625, 0.1, 0.25, 0.5, 0.9, 1.0, 1.5)      # the list of tests/test_gpu_fuzz.py (compared by the CPU test)
PENALTY_VALUES = (0.25, 0.5, 0.8, 1.0, 1.2, 2.0)
PADDED_DIMS = (1, 3, 5, 9, 12)
LENGTH_CLASSES = ((1, 3), (4, 63), (64, 65), (66, 256), (257, 330))
LENGTH_WEIGHTS = (0.2, 0.33, 0.15, 0.27, 0.05)
OPERATIONS = ("paths", "spot", "spot_hits", "spot_paths", "cross", "cross_linkage", "align_all", "medoids", "barycenters")
PUSH_SIZES = (0, 1, 2, 7, 33, 64, 65, 100)
HISTORIES = (0, 1, 7, 24, 64, 200)
CHANNEL_COLUMNS = 400
OUTCOMES = ("traced", "end aged out", "start aged out", "wrong start", "none")


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def spot_max_stream():
    m = re.search(r"constexpr\s+uint32_t\s+kSpotMaxStream\s*=\s*(0x[0-9A-Fa-f]+|\d+)u?\s*;", kt.header_text())
    return int(m.group(1), 0)


def fuzz_band_list():
    """The band percentages of tests/test_gpu_fuzz.py, read from its text."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_fuzz.py")) as f:
        m = re.search(r"pct = float\(rng\.choice\(\[([^\]]*)\]\)\)", f.read())
    return tuple(float(v) for v in m.group(1).split(","))


# ---- draws shared by both generators

def dimension_kind(dim, dims=None):
    dims = kt.parse_dims(kt.header_text()) if dims is None else dims
    return "kernel" if dim in dims else ("padded" if dim < max(dims) else "beyond")


def _draw_dim(rng):
    dims = kt.parse_dims(kt.header_text())
    top = max(dims)
    group = int(rng.integers(3))
    if group == 0:
        dim = int(rng.choice(dims))
    elif group == 1:
        dim = int(rng.choice([d for d in PADDED_DIMS if d not in dims]))
    else:
        dim = int(rng.choice([top + 1, top + 2, top + 3, top + 4, top + 14]))
    return dim, dimension_kind(dim, dims)


def _draw_penalties(rng):
    u = rng.random()
    if u < 0.35:
        return (1.0, 1.0, 1.0), "unit"
    if u < 0.55:
        return (0.7, 0.7, 0.7), "equal"
    return tuple(float(v) for v in rng.choice(PENALTY_VALUES, 3)), "drawn"


def _draw_length(rng, attempt):
    """A length by class; every failed attempt (a draw beyond the budget) makes the two long classes rarer."""
    w = np.array(LENGTH_WEIGHTS)
    w[3:] *= 0.75 ** attempt
    if attempt >= 12:
        w[2:] = 0.0
    lo, hi = LENGTH_CLASSES[int(rng.choice(len(w), p=w / w.sum()))]
    return int(rng.integers(lo, hi + 1))


def _values(rng, kind, n, dim):
    if kind == "gauss":
        return rng.standard_normal((n, dim)).astype(F)
    if kind == "integers":
        return rng.integers(0, 3, (n, dim)).astype(F)
    return (np.cumsum(rng.standard_normal((n, dim)), axis=0) * 0.4).astype(F)


def resident_dim(dim):
    """The D a spotting kernel of source dimension dim is instantiated with: the kernel dimension it pads to, or 0."""
    d = kt.kernel_dim(dim)
    return d if d in kt.parse_dims(kt.header_text()) else 0


def spot_class(dim, n):
    """(RT, D) of a query of n frames at source dimension dim."""
    d = resident_dim(dim)
    return (kt.spot_row_class(d, n) if d else 0), d


def band_cells(n, m, pct):
    """Cells of the checker's banded table of an n x m pair (tests/_path_reference.py::table)."""
    w = max(pref.band_from_pct(pct, max(n, m)), abs(n - m)) + 2
    i = np.arange(1, n + 1)
    return int(np.maximum(np.minimum(i + w, m + 1) - np.maximum(i - w, 1), 0).sum())


def path_half_width(n, m, pct):
    """host_w of csrc/apd_internal.h: the band, clamped to the longer sequence, widened to the length gap, plus 2."""
    return max(min(pref.band_from_pct(pct, max(n, m)), max(n, m)), abs(n - m)) + 2


def _chunks(costs, cap):
    """Chunks of the library's greedy planner: at least one item, then as many as keep every cost column at or under the cap."""
    chunks, at = 0, 0
    while at < len(costs):
        total = np.zeros(len(costs[0]), dtype=np.int64)
        first = at
        while at < len(costs) and (at == first or np.all(total + costs[at] <= cap)):
            total = total + costs[at]
            at += 1
        chunks += 1
    return chunks


def cap_for_chunks(costs):
    """A cap under which the planner cuts the list into 2 .. 4 chunks, or None (fewer than two items).  costs[p]: the byte counts
    the planner adds up for item p, one column per quantity it compares with the cap."""
    costs = [np.asarray(c, dtype=np.int64) for c in costs]
    if len(costs) < 2:
        return None
    need = int(np.sum(costs, axis=0).max())
    for cap in (need // 3, need // 2, need // 4, need - 1):
        if cap >= 1 and 2 <= _chunks(costs, cap) <= 4:
            return cap
    return None


def path_cap_costs(lengths, pairs, pct):
    """Per pair (direction bytes, step bytes) as apd_align_paths adds them up."""
    out = []
    for x, y in pairs:
        n, m = lengths[x], lengths[y]
        cells = max((2 * path_half_width(n, m, pct) + 1 + 63) // 64, 2)
        words = 0 if n < 2 or m < 2 else (n + 63) * ((cells + 15) // 16) * 64
        out.append((words * 4, (n + m - 1) * 16))
    return out


# ---- feature cases

def _draw_corpus(rng, attempt):
    n_seq = int(rng.integers(8, 17))
    n_streams = int(rng.integers(2, 5))
    q_lens = [_draw_length(rng, attempt) for _ in range(n_seq - n_streams)]
    s_lens = [int(rng.integers(1, 121)) for _ in range(n_streams)]
    copy = None
    if rng.random() < 0.3:                                          # one query will be an exact copy of another: the same length
        a, b = (int(v) for v in rng.choice(len(q_lens), 2, replace=False))
        q_lens[b] = q_lens[a]
        copy = (a, b)
    return q_lens, s_lens, copy


def _draw_ops(rng, form):
    counts = {op: int(rng.integers(0, 3)) for op in OPERATIONS}
    if not form.startswith("joined"):
        counts["cross"] = counts["cross_linkage"] = 0
    for dependent, provider in (("spot_hits", "spot"), ("spot_paths", "spot"), ("cross_linkage", "cross"), ("medoids", "align_all")):
        if counts[dependent] and not counts[provider]:
            counts[provider] = 1
    names = [op for op in OPERATIONS for _ in range(counts[op])]
    order = [names[i] for i in rng.permutation(len(names))] if names else []
    for dependent, provider in (("spot_hits", "spot"), ("spot_paths", "spot"), ("cross_linkage", "cross"), ("medoids", "align_all")):
        if dependent in order and order.index(dependent) < order.index(provider):       # the first provider moves ahead of it
            order.remove(provider)
            order.insert(order.index(dependent), provider)
    return order


def _partition(rng, members, n_sets):
    """`members` dealt into n_sets sets in a drawn order (unsorted inside), then one empty set at a drawn position."""
    members = [int(v) for v in rng.permutation(members)]
    cuts = sorted(int(v) for v in rng.integers(0, len(members) + 1, n_sets - 1))
    sets = [members[a:b] for a, b in zip([0] + cuts, cuts + [len(members)])]
    sets.insert(int(rng.integers(0, len(sets) + 1)), [])
    return sets


def _fill_ops(rng, order, lengths, queries, streams, n_first, form, pct):
    """The operations' own draws, from the lengths alone."""
    n = len(lengths)
    ops = []
    short = [s for s in range(n) if lengths[s] <= 130] or list(range(n))
    for at, name in enumerate(order):
        op = {"op": name}
        before = ops[:at]
        if name == "paths":
            count = int(rng.integers(1, 25))
            pool = short if rng.random() < 0.7 else list(range(n))
            pairs = [(int(rng.choice(pool)), int(rng.choice(pool))) for _ in range(count)]
            if count >= 3:
                pairs[-1] = pairs[0]                                                    # a repeat
                pairs[-2] = (pairs[1][0], pairs[1][0])                                  # (s, s)
            op["pairs"] = pairs
        elif name == "spot":
            count = int(rng.integers(2, 9))
            by_class = {}
            for q in queries:
                by_class.setdefault(kt.spot_rows_per_lane(lengths[q]), []).append(q)
            picks = [int(rng.choice(v)) for v in by_class.values()]                     # one query of every class there is
            picks = [picks[i] for i in rng.permutation(len(picks))][:count]
            while len(picks) < count:
                picks.append(int(rng.choice(queries)))
            pairs = [(q, int(rng.choice(streams))) for q in picks]
            pairs[-1] = pairs[0]                                                        # a repeat
            op["pairs"] = pairs
            drawn = bool(rng.random() < 0.7)                                            # a later spot_hits needs one curve before it
            op["curves"] = drawn or ("spot_hits" in order[at + 1:] and not any(o["op"] == "spot" and o["curves"] for o in before))
            op["via"] = "streams" if form.startswith("joined") and rng.random() < 0.5 else "own"
        elif name == "spot_hits":
            op["of"] = max(i for i, o in enumerate(before) if o["op"] == "spot" and o["curves"])
            op["pair"] = int(rng.integers(len(ops[op["of"]]["pairs"])))
        elif name == "spot_paths":
            op["of"] = max(i for i, o in enumerate(before) if o["op"] == "spot")
            k = len(ops[op["of"]]["pairs"])
            op["which"] = [int(v) for v in rng.permutation(k)[:3]]
            op["wrong"] = int(rng.integers(1 << 16))
        elif name == "cross":
            op["mode"] = ("hybrid", "exact", "strict")[int(rng.integers(3))]
        elif name == "cross_linkage":
            op["of"] = max(i for i, o in enumerate(before) if o["op"] == "cross")
            op["sets"] = _partition(rng, list(range(n - n_first)), int(rng.integers(1, 4)))
        elif name == "medoids":
            op["of"] = max(i for i, o in enumerate(before) if o["op"] == "align_all")
            op["sets"] = _partition(rng, list(range(n)), int(rng.integers(2, 4)))
        elif name == "barycenters":
            pool = [int(v) for v in rng.permutation(short)]
            size = int(rng.integers(2, 5))
            sets = [pool[:size], [], [int(rng.choice(short))]]                          # one set, one empty, one singleton
            if len(pool) >= size + 2 and rng.random() < 0.5:
                sets.append(pool[size:size + 2])
            sets = [sets[i] for i in rng.permutation(len(sets))]
            kind = ("member", "non-member", None)[int(rng.integers(3))]
            if kind is None and not any(o["op"] == "align_all" for o in before):
                kind = "member"
            init = []
            for s in sets:
                if not s:
                    init.append(0)
                elif kind == "non-member":
                    init.append(int(rng.choice([v for v in short if v not in s] or s)))
                else:
                    init.append(int(rng.choice(s)))
            op.update(sets=sets, init_kind=kind, init=None if kind is None else init, iterations=int(rng.choice([0, 1, 3])),
                      on_device=bool(rng.random() < 0.5), stream=int(rng.choice(streams)))
        ops.append(op)
    return ops


def feature_cells(lengths, ops, pct):
    """Checker DP cells of the case: every distinct (x, y) once per checker (banded path table, free-start curves, free-start
    table), every barycenter iteration, and the spot of an on-device barycenter."""
    paths, spots, tables, cells = set(), set(), set(), 0
    for op in ops:
        if op["op"] == "paths":
            paths.update(op["pairs"])
        elif op["op"] == "spot":
            spots.update(op["pairs"])
        elif op["op"] == "spot_paths":
            tables.update(ops[op["of"]]["pairs"][w] for w in op["which"])
            spots.update(ops[op["of"]]["pairs"][w] for w in op["which"])               # the windows come from the curves
        elif op["op"] == "barycenters":
            for s, members in enumerate(op["sets"]):
                if not members:
                    continue
                t = lengths[op["init"][s]] if op["init"] is not None else max(lengths[v] for v in members)
                cells += op["iterations"] * sum(band_cells(t, lengths[v], pct) for v in members)
            if op["on_device"]:
                t = max(lengths[v] for s in op["sets"] for v in s)
                cells += t * lengths[op["stream"]]
    cells += sum(band_cells(lengths[x], lengths[y], pct) for x, y in paths)
    cells += sum(lengths[x] * lengths[y] for x, y in spots) + sum(lengths[x] * lengths[y] for x, y in tables)
    return cells


_FEATURE = {}


def feature_case(seed, k, budget=CASE_BUDGET):
    """One corpus and its operations: a SimpleNamespace (see the module's docstring); the same object for the same arguments."""
    if (seed, k, budget) in _FEATURE:
        return _FEATURE[(seed, k, budget)]
    rng = _rng("feature", seed, k)
    dim, dim_kind = _draw_dim(rng)
    pens, pen_kind = _draw_penalties(rng)
    pct = float(rng.choice(BAND_PCTS))
    form = ("plain", "joined-AB", "joined-BA", "refilled")[int(rng.choice(4, p=[0.25, 0.25, 0.25, 0.25]))]
    value_kind = ("gauss", "integers", "walk")[int(rng.integers(3))]
    order = _draw_ops(rng, form)
    attempt = 0
    while True:
        sub = _rng("feature-lengths", seed, k, attempt)
        q_lens, s_lens, copy = _draw_corpus(sub, attempt)
        # A: the queries, B: the streams; the joined batch holds A then B, or B then A
        first, second = (s_lens, q_lens) if form == "joined-BA" else (q_lens, s_lens)
        lengths = list(first) + list(second)
        n_first = len(first)
        in_a = range(n_first, len(lengths)) if form == "joined-BA" else range(n_first)
        queries = list(in_a)
        streams = [s for s in range(len(lengths)) if s not in queries]
        ops = _fill_ops(sub, order, lengths, queries, streams, n_first, form, pct)
        cells = feature_cells(lengths, ops, pct)
        if cells <= budget:
            break
        attempt += 1
        assert attempt < 200, "no draw of (%r, %r) fits the budget" % (seed, k)
    seqs = [_values(rng, value_kind, n, dim) for n in lengths]
    if copy is not None:                                                                # an exact copy among the queries
        copy = (queries[copy[0]], queries[copy[1]])
        seqs[copy[1]] = seqs[copy[0]].copy()
    poison = None
    if rng.random() < 0.1:
        poison = ("nan frame", "inf component", "tiny sequence")[int(rng.integers(3))]
        s = int(rng.integers(len(seqs)))
        t = int(rng.integers(lengths[s]))
        if poison == "nan frame":
            seqs[s][t, :] = np.nan
        elif poison == "inf component":
            seqs[s][t, int(rng.integers(dim))] = F(np.inf) if rng.random() < 0.5 else F(-np.inf)
        else:
            seqs[s] = seqs[s] * F(2.0 ** -45)
    other = [rng.standard_normal(s.shape).astype(F) for s in seqs] if form == "refilled" else None
    caps = {}
    first_paths = next((op for op in ops if op["op"] == "paths"), None)
    first_spot = next((op for op in ops if op["op"] == "spot" and op["curves"]), None)
    for name, op in (("APD_PATH_WORKSPACE_BYTES", first_paths), ("APD_SPOT_WORKSPACE_BYTES", first_spot)):
        kind = ("unset", "one", "chunks")[int(rng.integers(3))]
        value = None
        if kind == "one":
            value = 1
        elif kind == "chunks":
            if op is not None and name == "APD_PATH_WORKSPACE_BYTES":
                value = cap_for_chunks(path_cap_costs(lengths, op["pairs"], pct))
            elif op is not None:
                value = cap_for_chunks([(8 * lengths[y],) for _, y in op["pairs"]])
            if value is None:
                kind = "unset"
        caps[name] = (kind, value)
    case = types.SimpleNamespace(seed=seed, k=k, dim=dim, dim_kind=dim_kind, pens=pens, pen_kind=pen_kind, pct=pct, form=form,
                                 value_kind=value_kind, seqs=seqs, lengths=lengths, n_first=n_first, queries=queries, streams=streams,
                                 other=other, poison=poison, copy=copy, caps=caps, ops=ops, cells=cells, attempts=attempt)
    _FEATURE[(seed, k, budget)] = case
    return case


def case_bytes(case):
    """Every input array of a case, as bytes."""
    parts = [s.tobytes() for s in case.seqs] + [s.tobytes() for s in (case.other or [])]
    return b"".join(parts)


def feature_triples(case):
    """The (kind, RT, D) a feature case must dispatch: a sweep per spotted query class, a recording sweep per pair a spot_paths
    asks a real window of (every pair it names: the best of a pair, or a wrong start, is one), a sweep for the on-device barycenter
    whose length is known ahead (an explicit init)."""
    out = set()
    for op in case.ops:
        if op["op"] == "spot":
            out.update(("sweep",) + spot_class(case.dim, case.lengths[x]) for x, _ in op["pairs"])
        elif op["op"] == "spot_paths":
            pairs = case.ops[op["of"]]["pairs"]
            out.update(("record",) + spot_class(case.dim, case.lengths[pairs[w][0]]) for w in op["which"])
        elif op["op"] == "barycenters" and op["on_device"] and op["init"] is not None:
            k = first_set(op["sets"])
            out.add(("sweep",) + spot_class(case.dim, case.lengths[op["init"][k]]))
    return out


def first_set(sets):
    """The first set with members: the one whose on-device barycenter is spotted."""
    return next(k for k, s in enumerate(sets) if s)


def spot_windows(case, op, reference):
    """[(x, y, end, start)] of a spot_paths operation, from the CHECKER's curves: per named pair its hits under the median score
    (at most four), its best, a {0, 0} record, one wrong start and one duplicate.  reference(x, y) -> (cost, start, best)."""
    records = []
    pairs = case.ops[op["of"]]["pairs"]
    for w in op["which"]:
        x, y = pairs[w]
        cost, start, best = reference(x, y)
        n = case.lengths[x]
        with np.errstate(all="ignore"):
            threshold = F(np.median(sref.scores(cost, start, n)))
        for h in sref.hits(cost, start, n, threshold)[:4]:
            records.append((x, y, int(h["end"]), int(h["start"])))
        records.append((x, y, int(best["end"]), int(best["start"])))
        records.append((x, y, 0, 0))
        end = 1 + op["wrong"] % len(cost)
        s = int(start[end - 1])
        records.append((x, y, end, s + 1 if s + 1 <= end else max(s - 1, 1)))
        records.append(records[-3 if best["end"] else -1])                              # a duplicate
    return records


# ---- stream scenarios

class StreamModel:
    """What the contract says of one session: a tests/_spot_stream_path_reference.py::Session per (query, channel), the frames of
    every channel since its reset (for the whole-stream checker), and the answers in the layout of the Python mirror."""

    def __init__(self, queries, channels, pens, history=0):
        self.queries, self.channels, self.pens = [np.asarray(q, dtype=F) for q in queries], int(channels), pens
        self.lens = [len(q) for q in self.queries]
        self.pairs = [[hist.Session(q, *pens, history=history) for q in self.queries] for _ in range(self.channels)]
        self.first = [0] * self.channels
        self.since = [[] for _ in range(self.channels)]
        self.H = int(history)

    def push(self, chunks):
        """(curves per pair p = channel * n_queries + q, best per pair)."""
        curves, best = [], np.zeros(self.channels * len(self.queries), dtype=sref.BEST)
        for c, chunk in enumerate(chunks):
            if len(chunk):
                self.since[c].append(np.asarray(chunk, dtype=F))
            for q, s in enumerate(self.pairs[c]):
                cost, start, b = s.push(chunk)
                curves.append((cost, start))
                best[c * len(self.queries) + q] = b
        return curves, best

    def reset(self, channel, first_column):
        for c in range(self.channels) if channel is None else [channel]:
            for s in self.pairs[c]:
                s.reset(first_column)
            self.first[c], self.since[c] = int(first_column), []

    def keep(self, history):
        self.H = int(history)
        for row in self.pairs:
            for s in row:
                s.keep(history)

    def columns(self, c):
        return self.pairs[c][0].column

    def history(self, c):
        return self.pairs[c][0].kept()

    def answer(self, window):
        q, c, end, start = (int(v) for v in window)
        return self.pairs[c][q].answer(end, start)

    def outcome(self, window):
        q, c, end, start = (int(v) for v in window)
        first, _ = self.history(c)
        steps, found, _ = self.answer(window)
        if end == 0 or start == 0:
            return "none"
        if end < first:
            return "end aged out"
        if len(steps):
            return "traced"
        return "start aged out" if found == start else "wrong start"

    def windows(self, rng, max_pairs=2):
        """The windows a `paths` action asks, from the rings: per drawn pair the last column and a drawn one (traced, or their
        start has aged out), an end that has aged out, a start that has aged out, one wrong start and {0, 0}."""
        out = []
        nq = len(self.queries)
        for p in rng.permutation(self.channels * nq)[:max_pairs]:
            c, q = int(p) // nq, int(p) % nq
            s = self.pairs[c][q]
            first, last = s.kept()
            fc = self.first[c]

            def start_of(end, s=s):
                return int(s.ring_c[end % s.H][1])

            if last >= first:
                for end in {last, int(rng.integers(first, last + 1))}:
                    if start_of(end):
                        out.append((q, c, end, start_of(end)))
                aged = [end for end in range(first, last + 1) if 0 < start_of(end) < first]
                if aged:
                    out.append((q, c, aged[-1], start_of(aged[-1])))
                found = start_of(last)
                wrong = found + 1 if found + 1 <= last else found - 1
                if found and wrong > fc:
                    out.append((q, c, last, wrong))
            if first - 1 >= fc + 1:
                out.append((q, c, first - 1, first - 1))
            out.append((q, c, 0, 0))
        return out


def _draw_actions(rng, sessions, n_actions, limit):
    """The actions without their windows, from counters alone: [(session, kind, arguments)], and the cells they cost."""
    col = [[0] * s["channels"] for s in sessions]                   # absolute column
    pushed = [[0] * s["channels"] for s in sessions]                # frames ever pushed: at most CHANNEL_COLUMNS
    hist_now = [s["history"] for s in sessions]
    after_reset = [False] * len(sessions)                           # the session's next push is the first after a reset of pushed data
    actions, cells = [], 0
    for _ in range(n_actions):
        s = int(rng.integers(len(sessions)))
        ch = sessions[s]["channels"]
        u = rng.random()
        if u < 0.5:
            sizes = []
            for c in range(ch):
                room = min(CHANNEL_COLUMNS - pushed[s][c], limit - 1 - col[s][c])
                sizes.append(int(rng.choice([v for v in PUSH_SIZES if v <= room])))
                col[s][c] += sizes[-1]
                pushed[s][c] += sizes[-1]
            cells += sum(sizes) * sum(sessions[s]["lens"])
            args = dict(sizes=sizes, curves=bool(rng.random() < 0.75), device=bool(rng.random() < 0.3), infinite=False)
            if after_reset[s] and sum(sizes):
                # An infinite component in the first frame behind a reset: every cell of that column is +INF, rows 2 .. n take MATCH
                # from column 0 and the curve shows the START column 0 holds -- the half of the reset state no finite stream reads.
                args["infinite"], args["curves"] = bool(rng.random() < 0.7), True
                after_reset[s] = False
            actions.append((s, "push", args))
        elif u < 0.62:
            channel = None if rng.random() < 0.3 else int(rng.integers(ch))
            fc = (0, 1000, limit - 10)[int(rng.choice(3, p=[0.4, 0.4, 0.2]))]
            for c in range(ch) if channel is None else [channel]:
                after_reset[s] = after_reset[s] or pushed[s][c] > 0
                col[s][c] = fc
            actions.append((s, "reset", dict(channel=channel, first_column=fc)))
        elif u < 0.74 or (u < 0.88 and not hist_now[s]):
            hist_now[s] = int(rng.choice(HISTORIES))
            actions.append((s, "keep", dict(history=hist_now[s])))
        elif u < 0.88:
            actions.append((s, "paths", dict(draw=int(rng.integers(1 << 30)))))
        elif u < 0.94:
            actions.append((s, "columns", {}))
        else:
            actions.append((s, "history", {}))
    return actions, cells


_STREAM = {}


def stream_case(seed, k, budget=CASE_BUDGET):
    """One streaming scenario: a SimpleNamespace with the templates, the two sessions' (queries, channels, history) and the actions
    [dict(session, kind, ..., want)]; `want` is the model's word on the action.  The same object for the same arguments."""
    if (seed, k, budget) in _STREAM:
        return _STREAM[(seed, k, budget)]
    rng = _rng("stream", seed, k)
    dim, dim_kind = _draw_dim(rng)
    pens, pen_kind = _draw_penalties(rng)
    value_kind = ("gauss", "integers", "walk")[int(rng.integers(3))]
    n_queries = int(rng.integers(2, 5))
    limit = spot_max_stream()
    attempt = 0
    while True:
        sub = _rng("stream-lengths", seed, k, attempt)
        lengths = [1] + [_draw_length(sub, attempt) for _ in range(n_queries - 1)]
        lengths = [lengths[i] for i in sub.permutation(n_queries)]
        one = list(range(n_queries))
        two = [int(v) for v in sub.integers(0, n_queries, int(sub.integers(1, 4)))]                 # other queries, repeats allowed
        sessions = [dict(queries=one, channels=int(sub.integers(1, 4)), history=int(sub.choice(HISTORIES))),
                    dict(queries=two, channels=int(sub.integers(1, 4)), history=int(sub.choice(HISTORIES)))]
        if sessions[1]["queries"] == one and sessions[1]["channels"] == sessions[0]["channels"]:
            sessions[1]["channels"] = sessions[0]["channels"] % 3 + 1                               # the second session is another one
        for s in sessions:
            s["lens"] = [lengths[q] for q in s["queries"]]
        skeleton, cells = _draw_actions(sub, sessions, int(sub.integers(12, 26)), limit)
        if cells <= budget:
            break
        attempt += 1
        assert attempt < 200, "no draw of (%r, %r) fits the budget" % (seed, k)
    templates = [_values(rng, value_kind, n, dim) for n in lengths]
    models = [StreamModel([templates[q] for q in s["queries"]], s["channels"], pens, s["history"]) for s in sessions]
    actions = []
    for s, kind, args in skeleton:
        model = models[s]
        act = dict(session=s, kind=kind, **args)
        if kind == "push":
            act["chunks"] = [_values(rng, value_kind, n, dim) for n in args["sizes"]]
            if args["infinite"]:
                for c, chunk in enumerate(act["chunks"]):
                    if len(chunk):
                        chunk[0, c % dim] = F(np.inf) if c % 2 == 0 else F(-np.inf)
            curves, best = model.push(act["chunks"])
            act["want"] = dict(curves=curves, best=best)
        elif kind == "reset":
            model.reset(args["channel"], args["first_column"])
            act["want"] = {}
        elif kind == "keep":
            model.keep(args["history"])
            act["want"] = {}
        elif kind == "paths":
            assert model.H > 0
            act["windows"] = model.windows(_rng("stream-windows", seed, k, args["draw"]))
            act["want"] = dict(answers=[model.answer(w) for w in act["windows"]], outcomes=[model.outcome(w) for w in act["windows"]])
        else:
            act["want"] = {}
        act["want"]["columns"] = [model.columns(c) for c in range(model.channels)]
        act["want"]["history"] = [model.history(c) for c in range(model.channels)]
        act["want"]["H"] = model.H
        if kind == "paths":                                                             # the state the whole-stream checker needs
            act["want"]["whole"] = _whole_state(model)
        actions.append(act)
    case = types.SimpleNamespace(seed=seed, k=k, dim=dim, dim_kind=dim_kind, pens=pens, pen_kind=pen_kind, value_kind=value_kind,
                                 templates=templates, lengths=lengths, sessions=sessions, actions=actions, cells=cells,
                                 attempts=attempt)
    _STREAM[(seed, k, budget)] = case
    return case


def _whole_state(model):
    """A frozen copy of what whole_answer reads: per channel (first column, frames since the reset, kept)."""
    return [(model.first[c], [a for a in model.since[c]], model.history(c)) for c in range(model.channels)]


def whole_answer(case, act, t):
    """The whole-stream checker's answer to window t of a `paths` action: _spot_path_reference.answer on the stream since the
    channel's reset, through _spot_stream_path_reference.expected, from the state frozen beside the action."""
    q, c, end, start = (int(v) for v in act["windows"][t])
    fc, since, kept = act["want"]["whole"][c]
    session = case.sessions[act["session"]]
    x = case.templates[session["queries"][q]]
    n = len(x)
    key = (id(act), q, c)
    if key not in _TABLES:
        _TABLES.clear()                                                                  # one table at a time
        _TABLES[key] = spref.table(x, np.concatenate(since, axis=0), *case.pens) if since else None
    tab = _TABLES[key]
    if tab is None or end == 0 or start == 0 or end <= fc:
        found = hist.NONE
    else:
        found = spref.answer(tab, n, end - fc, start - fc)
    return hist.expected(found, n, fc, kept, end, start)


_TABLES = {}


def stream_bytes(case):
    parts = [t.tobytes() for t in case.templates]
    for act in case.actions:
        if act["kind"] == "push":
            parts += [c.tobytes() for c in act["chunks"]]
        if act["kind"] == "paths":
            parts.append(np.array(act["windows"], dtype=np.int64).tobytes())
    return b"".join(parts)


def stream_triples(case):
    """The (kind, RT, D) a stream scenario must dispatch: per push with a frame, every query class of its session, as a plain or a
    recording streaming sweep by the history in force."""
    out = set()
    for act in case.actions:
        if act["kind"] == "push" and sum(act["sizes"]):
            kind = "streamrec" if act["want"]["H"] else "stream"
            out.update((kind,) + spot_class(case.dim, n) for n in case.sessions[act["session"]]["lens"])
    return out


def describe(act):
    """An action without its arrays, for the determinism test and for messages."""
    return {k: v for k, v in act.items() if k not in ("chunks", "want")}
