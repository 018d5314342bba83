"""Seeded random sweep of everything built after apd_align_all and UPGMA -- warping paths, cross matrices and linkage, medoids and
barycenters, spotting with its hits and window paths, streaming sessions with and without a history -- on ONE context per test
function, against the checkers of the feature modules.  tests/_feature_cases.py draws the cases (and tests/test_feature_cases.py
shows, without a GPU, what the committed seeds cover and that they fit the budget of checker cells); tools/debug/fuzz_features.py is
the open-ended version and the replay of a single case.

What the feature modules cannot see and this one can: a context serves every feature through workspaces that are never cleared and a
tile-plan cache, so a kernel that relies on what a fresh allocation holds, or reads what another feature's call left behind, passes
every module that makes its own context and calls its own feature.  Here the operations of a case run in a drawn order, the cases of
a seed run one after the other on the same context, and the workspace caps change from case to case.

Every promise is bits, so there is no tolerance here but the 1e-4 of the default distance mode (align_all and cross in hybrid or
exact mode with equal penalties on a corpus inside the fast feature range: tests/test_gpu_cross.py::assert_parity); everything else
is compared bit for bit, NaN payloads aside.  The Python mirror is what is driven (AlignmentWorkers, SpotStream, clustering.*)."""
import warnings

import numpy as np
import pytest

import _dba_reference as dba
import _feature_cases as fc
import _kernel_table as kt
import _linkage_reference as lref
import _path_reference as pref
import _spot_path_reference as spref
import _spot_reference as sref
from test_gpu_cross import assert_bitwise, assert_parity, pack
from test_gpu_dtw import _assert_same_bits_or_nan
from test_gpu_paths import assert_same_path
from test_gpu_prototypes import assert_same as assert_same_prototypes
from test_gpu_spot import assert_same as assert_same_spot
from test_gpu_spot_stream_paths import same_window

pytestmark = pytest.mark.gpu
F = np.float32
_seen = set()                                   # (kind, RT, D) of every spotting-kernel line read in this module
_ran = set()                                    # ("feature" | "stream", seed) of the sweeps that ran to their end


def replay(kind, seed, k, index):
    return "seed %d case %d %s %d; replay: python tools/debug/fuzz_features.py --replay %s%d:%d:%d" % (
        seed, k, "operation" if kind == "feature" else "action", index, "" if kind == "feature" else "stream:", seed, k, index)


def discovery(pct, pens):
    from audio_pattern_discovery_amd.discovery import Discovery
    return Discovery(warping_band_percentage=pct, insertion_penalty=pens[0], deletion_penalty=pens[1], match_penalty=pens[2])


# ---- one feature case

class Corpus:
    """The GPU side of a feature case: the workers over all its sequences in the case's batch form, and, for the joined forms, the
    workers of the two sets."""

    def __init__(self, ctx, case):
        from audio_pattern_discovery_amd import _lib
        from audio_pattern_discovery_amd.alignments import AlignmentWorkers, Batch, NDSequence
        import ctypes as C
        self.ctx, self.first, self.second = ctx, None, None
        nd = [NDSequence(s) for s in case.seqs]
        if case.form == "refilled":                                                     # other values of the same lengths, then the case's
            self.all = AlignmentWorkers.new([NDSequence(s) for s in case.other], ctx)
            frames, _ = pack(case.seqs, case.dim)
            _lib.check(_lib.lib().apd_batch_refill(ctx.handle, self.all._batch.handle, C.c_void_p(frames.ctypes.data), 0), ctx.handle)
            self.all.data = nd
        elif case.form.startswith("joined"):
            self.first = AlignmentWorkers.new(nd[:case.n_first], ctx)
            self.second = AlignmentWorkers.new(nd[case.n_first:], ctx)
            self.all = AlignmentWorkers.new(nd, ctx)
            self.all._batch.close()
            self.all._batch = Batch.join(self.first._batch, self.second._batch)
        else:
            self.all = AlignmentWorkers.new(nd, ctx)

    def close(self):
        for w in (self.all, self.second, self.first):
            if w is not None:
                w.close()


def compare_matrix(got, want, case, bitwise, what):
    """The rule of a score matrix: bits in strict mode, under unequal penalties and on a corpus that leaves the fast feature range
    (every pair then runs the literal kernel: tests/test_gpu_dtw.py::test_nonfinite_features_follow_the_reference_select);
    tests/test_gpu_cross.py::assert_parity otherwise."""
    flagged = kt.leaves_fast_range(np.concatenate(case.seqs, axis=0))
    try:
        if flagged:
            _assert_same_bits_or_nan(got, want)
        elif bitwise or not (case.pens[0] == case.pens[1] == case.pens[2]):
            assert_bitwise(got, want, what)
        else:
            assert_parity(got, want, what)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (what, e)) from None


def run_feature_case(ctx, oracle, case, setenv, stop_after=None):
    """Runs the operations of one case in their order on `ctx` and compares each with its checker; AssertionError names the
    operation and its replay command.  setenv(name, value or None) sets or removes an environment variable."""
    from audio_pattern_discovery_amd import clustering
    from audio_pattern_discovery_amd.alignments import SPOT_BEST, AlignmentWorkers, Batch, NDSequence, spot_hits
    for name, (_, value) in case.caps.items():
        setenv(name, None if value is None else str(value))
    params = discovery(case.pct, case.pens)
    seqs, lengths, pens = case.seqs, case.lengths, case.pens
    frames, offsets = pack(seqs, case.dim)
    paths_of, curves_of, tables_of, results = {}, {}, {}, {}

    def curve(x, y):
        if (x, y) not in curves_of:
            curves_of[(x, y)] = sref.spot(seqs[x], seqs[y], *pens)
        return curves_of[(x, y)]

    ctx.set_distance_mode("hybrid")
    corpus = Corpus(ctx, case)
    W = corpus.all
    try:
        for i, op in enumerate(case.ops):
            if stop_after is not None and i > stop_after:
                break
            what = "%s (%s)" % (replay("feature", case.seed, case.k, i), op["op"])
            if op["op"] == "paths":
                got, scores = W.paths(op["pairs"], params)
                for p, (x, y) in enumerate(op["pairs"]):
                    if (x, y) not in paths_of:
                        paths_of[(x, y)] = pref.path(seqs[x], seqs[y], pref.band_from_pct(case.pct, max(lengths[x], lengths[y])), *pens)
                    assert_same_path(got[p], scores[p], *paths_of[(x, y)], "%s pair %d %s" % (what, p, (x, y)))
            elif op["op"] == "spot":
                if op["via"] == "streams":
                    curves, best = corpus.first.spot(op["pairs"], params, curves=op["curves"], streams=corpus.second)
                else:
                    curves, best = W.spot(op["pairs"], params, curves=op["curves"])
                assert len(best) == len(op["pairs"]) and len(curves) == (len(op["pairs"]) if op["curves"] else 0), what
                for p, (x, y) in enumerate(op["pairs"]):
                    assert_same_spot(curves[p] if op["curves"] else None, best[p], curve(x, y), "%s pair %d %s" % (what, p, (x, y)))
                results[i] = curves
            elif op["op"] == "spot_hits":
                x, _ = case.ops[op["of"]]["pairs"][op["pair"]]
                cost, start = results[op["of"]][op["pair"]]
                with np.errstate(all="ignore"), warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    threshold = F(np.median(sref.scores(cost, start, lengths[x])))
                got, want = spot_hits(cost, start, lengths[x], threshold), sref.hits(cost, start, lengths[x], threshold)
                assert len(got) == len(want) and sref.same_best(got, want), "%s pair %d threshold %r" % (what, op["pair"], threshold)
            elif op["op"] == "spot_paths":
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    records = fc.spot_windows(case, op, curve)
                windows = np.zeros(len(records), dtype=SPOT_BEST)
                windows["end"], windows["start"] = [r[2] for r in records], [r[3] for r in records]
                pairs = [(r[0], r[1]) for r in records]
                if case.ops[op["of"]]["via"] == "streams":
                    got, found, scores = corpus.first.spot_paths(pairs, windows, params, streams=corpus.second)
                else:
                    got, found, scores = W.spot_paths(pairs, windows, params)
                for t, (x, y, end, start) in enumerate(records):
                    if (x, y) not in tables_of:
                        tables_of.clear()                                               # one table at a time: the windows come pair by pair
                        tables_of[(x, y)] = spref.table(seqs[x], seqs[y], *pens)
                    want = spref.answer(tables_of[(x, y)], lengths[x], end, start)
                    assert same_window((got[t], found[t], scores[t]), want), "%s window %d %s" % (what, t, records[t])
            elif op["op"] == "cross":
                from test_gpu_cross import oracle_cross
                want_fs, want_sf = oracle_cross(oracle, ("sweep", case.seed, case.k), seqs[:case.n_first], seqs[case.n_first:], case.dim,
                                                case.pct, pens)
                ctx.set_distance_mode(op["mode"])
                try:
                    fs, sf = corpus.first.cross(corpus.second, params)
                finally:
                    ctx.set_distance_mode("hybrid")
                compare_matrix(fs, want_fs, case, op["mode"] == "strict", "%s %s fs" % (what, op["mode"]))
                compare_matrix(sf, want_sf, case, op["mode"] == "strict", "%s %s sf" % (what, op["mode"]))
                results[i] = (fs, sf)
            elif op["op"] == "cross_linkage":
                fs, sf = results[op["of"]]
                got = clustering.cross_linkage(fs, sf, op["sets"], ctx)
                lref.assert_equal(got, lref.reference(fs, sf, op["sets"]), what)
            elif op["op"] == "align_all":
                got = W.align_all(params).reshape(len(seqs), len(seqs)).copy()
                compare_matrix(got, oracle.align_all(frames, offsets, case.pct, *pens, workers=8), case, False, what)
                results[i] = got
            elif op["op"] == "medoids":
                medoid, cost = clustering.medoids(results[op["of"]], op["sets"], ctx)
                want_medoid, want_cost = dba.medoids(results[op["of"]], op["sets"])
                assert np.array_equal(medoid, want_medoid), "%s medoids %r, not %r" % (what, medoid, want_medoid)
                assert np.array_equal(pref.bits(cost), pref.bits(want_cost)), "%s medoid costs" % what
            elif op["op"] == "barycenters":
                init = op["init"]
                if init is None:                                                        # the medoids of the last align_all, as the mirror takes them
                    init = dba.medoids(W.result.reshape(len(seqs), len(seqs)), op["sets"])[0].copy()
                    init[init == dba.NONE] = 0
                want = dba.barycenters(seqs, op["sets"], init, case.pct, pens, op["iterations"])
                if not op["on_device"]:
                    got = W.barycenters(op["sets"], params, init=op["init"], iterations=op["iterations"])
                    assert_same_prototypes(got, want, what)
                    continue
                buf, off, inertia, used = W.barycenters(op["sets"], params, init=op["init"], iterations=op["iterations"], on_device=True)
                try:
                    flat = buf.to_numpy(F, int(off[-1]) * case.dim).reshape(-1, case.dim)
                    got = [flat[int(off[s]):int(off[s + 1])] for s in range(len(op["sets"]))]
                    assert_same_prototypes((got, inertia, used), want, what)
                    s = fc.first_set(op["sets"])                                        # that barycenter, resident, against one stream
                    proto = AlignmentWorkers.new([NDSequence(got[s])], ctx)
                    proto._batch.close()
                    proto._batch = Batch(ctx, buf.ptr + int(off[s]) * case.dim * 4, [0, len(got[s])], case.dim, on_device=True)
                    stream = AlignmentWorkers.new([NDSequence(seqs[op["stream"]])], ctx)
                    try:
                        curves, best = proto.spot([(0, 1)], params, streams=stream)
                    finally:
                        stream.close()
                        proto.close()
                    assert_same_spot(curves[0], best[0], sref.spot(want[0][s], seqs[op["stream"]], *pens), what + " spot of the barycenter")
                finally:
                    buf.free()
    finally:
        corpus.close()


# ---- one stream scenario

def run_stream_case(ctx, case, stop_after=None):
    """Applies the actions of a scenario to its two live sessions and compares, after every action, what the session returns and
    reports with the model's word recorded beside the action."""
    from audio_pattern_discovery_amd.alignments import SPOT_WINDOW, AlignmentWorkers, NDSequence
    params = discovery(1.0, case.pens)
    workers = AlignmentWorkers.new([NDSequence(t) for t in case.templates], ctx)
    sessions = []
    try:
        for s in case.sessions:
            sessions.append(workers.spot_stream(s["queries"], params, channels=s["channels"], history=s["history"]))
        for a, act in enumerate(case.actions):
            if stop_after is not None and a > stop_after:
                break
            what = "%s (%s)" % (replay("stream", case.seed, case.k, a), fc.describe(act))
            session, want = sessions[act["session"]], act["want"]
            if act["kind"] == "push":
                if act["device"]:
                    host = np.ascontiguousarray(np.concatenate(act["chunks"], axis=0))
                    buf = ctx.upload(host) if host.size else ctx.alloc(16)
                    chunk_off = np.concatenate([[0], np.cumsum(act["sizes"])]).astype(np.uint64)
                    try:
                        curves, best = session.push((buf.ptr, chunk_off), curves=act["curves"], on_device=True)
                    finally:
                        buf.free()
                else:
                    curves, best = session.push(act["chunks"], curves=act["curves"])
                assert len(curves) == (len(want["curves"]) if act["curves"] else 0), what
                for p, (cost, start) in enumerate(curves):
                    assert np.array_equal(start, want["curves"][p][1]), "%s pair %d start" % (what, p)
                    assert np.array_equal(sref.bits(cost), sref.bits(want["curves"][p][0])), "%s pair %d cost" % (what, p)
                assert sref.same_best(best, want["best"]), "%s best %r, not %r" % (what, best, want["best"])
            elif act["kind"] == "reset":
                session.reset(act["channel"], act["first_column"])
            elif act["kind"] == "keep":
                session.keep(act["history"])
            elif act["kind"] == "paths":
                got, found, scores = session.paths(np.array([tuple(w) for w in act["windows"]], dtype=SPOT_WINDOW))
                for t, w in enumerate(act["windows"]):
                    assert same_window((got[t], found[t], scores[t]), want["answers"][t]), "%s window %d %s (%s)" % (
                        what, t, w, want["outcomes"][t])
            for c in range(case.sessions[act["session"]]["channels"]):
                assert session.columns(c) == want["columns"][c], "%s columns of channel %d" % (what, c)
                assert session.history(c) == tuple(want["history"][c]), "%s history of channel %d" % (what, c)
    finally:
        for session in sessions:
            session.close()
        workers.close()


# ---- the sweeps

@pytest.mark.parametrize("seed", fc.FEATURE_SEEDS)
def test_features_interleaved_on_one_context(apd, oracle, capfd, monkeypatch, seed):
    setenv = lambda name, value: monkeypatch.delenv(name, raising=False) if value is None else monkeypatch.setenv(name, value)
    ctx = apd.Context(0)
    try:
        for k in range(fc.FEATURE_CASES_PER_SEED):
            with kt.debug_plan(capfd) as err:
                run_feature_case(ctx, oracle, fc.feature_case(seed, k), setenv)
            _seen.update(kt.read_spot_plan(err[0]))
    finally:
        ctx.close()
    _ran.add(("feature", seed))


@pytest.mark.parametrize("seed", fc.STREAM_SEEDS)
def test_stream_sessions_follow_the_model(apd, capfd, seed):
    ctx = apd.Context(0)
    try:
        for k in range(fc.STREAM_CASES_PER_SEED):
            with kt.debug_plan(capfd) as err:
                run_stream_case(ctx, fc.stream_case(seed, k))
            _seen.update(kt.read_spot_plan(err[0]))
    finally:
        ctx.close()
    _ran.add(("stream", seed))


def test_the_sweep_reached_the_kernels_it_was_drawn_for():
    """The union of the spotting kernels' own lines over the two sweeps above holds every (kind, RT, D) the generator predicts, on
    the CPU, from the drawn lengths and dimensions: a sweep that silently stopped reaching a class fails here, and so does a run of
    this test without the sweeps."""
    assert _ran == {("feature", s) for s in fc.FEATURE_SEEDS} | {("stream", s) for s in fc.STREAM_SEEDS}, "the sweeps did not all run"
    want = set()
    for seed in fc.FEATURE_SEEDS:
        for k in range(fc.FEATURE_CASES_PER_SEED):
            want |= fc.feature_triples(fc.feature_case(seed, k))
    for seed in fc.STREAM_SEEDS:
        for k in range(fc.STREAM_CASES_PER_SEED):
            want |= fc.stream_triples(fc.stream_case(seed, k))
    assert {t[0] for t in want} == {"sweep", "record", "stream", "streamrec"}
    assert want <= _seen, "predicted and never dispatched: %r" % sorted(want - _seen)
