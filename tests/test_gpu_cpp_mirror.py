"""The C++ mirror of the reference's Rust surface (include/apd.hpp) driven by tests/cpp/harness.cpp: the reference's call sequence vs
the oracle, and one harness mode per group of wrappers the reference does not have, bit for bit vs the CPU checkers."""
import os
import subprocess

import numpy as np
import pytest

from audio_pattern_discovery_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_end_to_end(oracle, tmp_path):
    exe = os.path.join(ROOT, "build", "apd_cpp_harness")
    if not os.path.exists(exe):
        pytest.fail("build/apd_cpp_harness missing: __graft_entry__.build() compiles it")
    n, dim, pct, perc = 14, 13, 0.0625, 0.2
    frames, offsets = synth.make_sequences(n, 40, dim, seed=31, copies=0.5)
    with open(tmp_path / "in.txt", "w") as fp:
        fp.write("%d %d %r 1.0 1.0 1.0 %r\n" % (n, dim, pct, perc))
        for s in synth.split(frames, offsets):
            fp.write("%d\n%s\n" % (len(s), " ".join(repr(float(v)) for v in s.ravel())))
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "audio_pattern_discovery_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe, str(tmp_path / "in.txt")], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    dist = np.array(lines[0].split()[1:], dtype=np.float32).reshape(n, n)
    want = oracle.align_all(frames, offsets, pct, workers=4)
    np.testing.assert_allclose(dist, want, rtol=1e-4, atol=0)
    # clustering is compared on the GPU's own matrix (bit-exact vs the literal algorithm on identical input)
    ops, roots, _ = oracle.clustering(dist, n, perc)
    got_ops = [tuple(l.split()[1:4]) + (l.split()[5],) for l in lines if l.startswith("op ")]
    assert got_ops == [(str(o["merge_i"]), str(o["merge_j"]), str(o["into"]), str(oracle.MERGE_NAMES.index(o["operation"]))) for o in ops]
    assert [int(v) for v in [l for l in lines if l.startswith("roots")][0].split()[1:]] == roots
    sets = [[int(v) for v in l.split()[1:]] for l in lines if l.startswith("set")]
    assert sets == oracle.cluster_sets(ops, roots, n)
    pair = float([l for l in lines if l.startswith("pair01")][0].split()[1])
    assert abs(pair - want[0, 1]) <= 1e-4 * want[0, 1]
    assert [l for l in lines if l.startswith("multi ")][0].split()[1:] == ["1", "1"]     # the multi-device handle on {0}: one rank, same bits
    assert [l for l in lines if l.startswith("multi_again")][0].split()[1:] == ["1", "rccl"]   # kept handle, second call, RCCL collective
    assert [l for l in lines if l.startswith("onecall")][0].split()[1:] == ["1", "1"]     # apd_dtw_all_pairs / apd_upgma: same bits


def test_cpp_mirror_with_the_references_on_disk_artefacts(oracle, tmp_path):
    """apd::AutoEncoder::from_file (bincode auto_encoder.bin, neural.rs:30-36) -> encoded() -> align_all -> clustering ->
    apd::dendrograms, parameters from apd::Discovery::from_toml (discovery.rs:28-36): main.rs:142-203 through the C++ mirror.
    PARITY UNPINNED for the file formats: no reference-made file exists; the weight file is written by the Python mirror's
    writer (same C entry point) and by hand-packed bytes in tests/test_host_abi.py."""
    import struct
    exe = os.path.join(ROOT, "build", "apd_cpp_harness")
    if not os.path.exists(exe):
        pytest.fail("build/apd_cpp_harness missing: __graft_entry__.build() compiles it")
    n, dim, latent, pct, perc = 12, 13, 8, 0.25, 0.5
    frames, offsets = synth.make_sequences(n, 36, dim, seed=77, copies=0.5)
    rng = np.random.default_rng(5)
    w = ((rng.random((dim, latent)) - 0.5) / latent).astype(np.float32)
    b = ((rng.random(latent) - 0.5) / latent).astype(np.float32)
    wd = rng.standard_normal((latent, dim)).astype(np.float32)
    bd = rng.standard_normal(dim).astype(np.float32)
    blob = b""
    for m, cols in ((w, latent), (wd, dim), (b, latent), (bd, dim)):                 # hand-packed bincode 1.x image
        blob += struct.pack("<Q", m.size) + m.astype("<f4").tobytes() + struct.pack("<Q", cols)
    (tmp_path / "auto_encoder.bin").write_bytes(blob)
    (tmp_path / "Discovery.toml").write_text(
        "dft_win = 256\ndft_step = 128\nceps_filter = 18\nauto_encoder = %d\nlearning_rate = 0.1\nepochs = 25\nepoch_drop = 5.0\n"
        "drop = 0.5\nvat_moving = 15\nvat_percentile = 0.95\nvat_min_len = 150\nwarping_band_percentage = %r  # band\n"
        "insertion_penalty = 1.0\ndeletion_penalty = 1.0\nmatch_penalty = 1.0\nalignment_workers = 4\nclustering_percentile = %r\n"
        % (latent, pct, perc))
    with open(tmp_path / "in.txt", "w") as fp:
        fp.write("%d %d 1.0 1.0 1.0 1.0 0.05\n" % (n, dim))                        # overridden by the TOML file
        for s_ in synth.split(frames, offsets):
            fp.write("%d\n%s\n" % (len(s_), " ".join(repr(float(v)) for v in s_.ravel())))
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "audio_pattern_discovery_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe, str(tmp_path / "in.txt"), str(tmp_path / "auto_encoder.bin"), str(tmp_path / "Discovery.toml")],
                         capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    get = lambda key: [l for l in lines if l.startswith(key + " ")][0].split()[1:]
    toml = get("toml")
    assert [int(toml[k]) for k in (0, 1, 2, 3, 5, 6, 12, 14)] == [256, 128, 18, 15, 150, 4, latent, 25]
    assert np.float32(toml[8]) == np.float32(pct) and np.float32(toml[7]) == np.float32(perc)
    assert get("latent") == [str(latent)] and get("roundtrip") == ["1"]
    enc = oracle.encode(frames, w, b)
    np.testing.assert_allclose(np.array(get("enc0"), np.float32).reshape(-1, latent), enc[:int(offsets[1])], rtol=1e-5, atol=1e-5)
    dist = np.array(get("dist"), dtype=np.float32).reshape(n, n)
    np.testing.assert_allclose(dist, oracle.align_all(enc, offsets, pct, workers=4), rtol=1e-4, atol=1e-6)
    ops, roots, _ = oracle.clustering(dist, n, float(np.float32(perc)))
    labels = ["{img%d}" % i for i in range(n)]
    results = {}
    for o in ops:
        i, j, k = o["merge_i"], o["merge_j"], o["into"]
        left = results[i] if o["operation"] in ("Cluster2Sequence", "Cluster2Cluster") else labels[i]
        right = results[j] if o["operation"] in ("Sequence2Cluster", "Cluster2Cluster") else labels[j]
        results[k] = "[.%d [%s %s ] ]" % (k, left, right)
    got = {int(l.split(" ", 2)[1]): l.split(" ", 2)[2] for l in lines if l.startswith("dendro ")}
    assert got == {r: results[r] for r in roots if r in results}


# ---- the wrappers that are not in the reference: one harness mode each (tests/cpp/harness.cpp says what a mode reads and prints),
# every float as its bits, compared bit for bit with the CPU checkers of the features.  tests/test_cpp_harness_coverage.py keeps the
# harness in step with the header.

F = np.float32
UNIT = (1.0, 1.0, 1.0)
SPOT_SKEWED = (1.0, 2.0, 0.5)                   # (insertion, deletion, match), tests/_spot_matrix.py
PATH_SKEWED = (1.5, 0.75, 1.25)                 # tests/test_gpu_prototypes.py


def hx(values):
    return " ".join("%08x" % b for b in np.ascontiguousarray(values, dtype=F).ravel().view(np.uint32))


def header_text(pct, pen, dim):
    return "%s %d\n" % (hx([pct] + list(pen)), dim)


def set_text(seqs):
    return "%d\n" % len(seqs) + "".join("%d\n%s\n" % (len(s), hx(s)) for s in seqs)


def sets_text(sets):
    return " ".join(["%d" % len(sets)] + ["%d %s" % (len(s), " ".join(str(m) for m in s)) for s in sets])


def windows_text(windows):
    return " ".join(["%d" % len(windows)] + ["%d %d %d %d" % tuple(w) for w in windows])


class Output:
    """What a mode printed, read in order: take(key) is the next line, which must begin with `key`."""

    def __init__(self, text):
        self.lines, self.at = [line.split() for line in text.splitlines()], 0

    def take(self, key):
        assert self.at < len(self.lines), "the output ends before `%s`" % key
        line = self.lines[self.at]
        assert line[0] == key, "line %d: expected `%s`, got %r" % (self.at, key, line[:6])
        self.at += 1
        return line[1:]

    def ints(self, key):
        return [int(t) for t in self.take(key)]

    def u32(self, key):
        return np.array(self.ints(key), dtype=np.uint32)

    def f32(self, key):
        return np.array([int(t, 16) for t in self.take(key)], dtype=np.uint32).view(F)

    def steps(self, count):
        import _path_reference as pr
        out = np.zeros(count, dtype=pr.STEP)
        for k in range(count):
            i, j, cost, op = self.take("step")
            out[k]["i"], out[k]["j"], out[k]["op"] = int(i), int(j), int(op)
            out["cost"].view(np.uint32)[k] = int(cost, 16)
        return out

    def best(self):
        import _spot_reference as sp
        end, start, cost, score = self.take("best")
        out = np.zeros(1, dtype=sp.BEST)
        out["end"], out["start"] = int(end), int(start)
        out["cost"].view(np.uint32)[0], out["score"].view(np.uint32)[0] = int(cost, 16), int(score, 16)
        return out[0]

    def spotted(self, key):
        """([best per pair], [(cost, start) per pair with curves])"""
        pairs, with_curves = self.ints(key)
        bests = [self.best() for _ in range(pairs)]
        return bests, [(self.f32("cost"), self.u32("start")) for _ in range(with_curves)]

    def paths(self):
        """[(steps, found_start, score as a one-element array)] per window"""
        (count,) = self.ints("paths")
        out = []
        for _ in range(count):
            found, score, used = self.take("window")
            out.append((self.steps(int(used)), int(found), np.array([int(score, 16)], dtype=np.uint32).view(F)))
        return out

    def done(self):
        assert self.at == len(self.lines), "unread output: %r" % self.lines[self.at][:6]


def run_mode(mode, text, tmp_path):
    exe = os.path.join(ROOT, "build", "apd_cpp_harness")
    if not os.path.exists(exe):
        pytest.fail("build/apd_cpp_harness missing: __graft_entry__.build() compiles it")
    (tmp_path / "in.txt").write_text(text)
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "audio_pattern_discovery_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe, mode, str(tmp_path / "in.txt")], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, "%s mode: exit %d\n%s%s" % (mode, out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    return Output(out.stdout)


def gauss(lengths, dim, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, dim)).astype(F) for n in lengths]


def same_f32(got, want):
    import _path_reference as pr
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    return got.shape == want.shape and np.array_equal(pr.bits(got), pr.bits(want))


def same_window(got, want):
    import _spot_path_reference as spp
    return spp.same_steps(got[0], want[0]) and int(got[1]) == int(want[1]) and same_f32(got[2], F(want[2]))


def test_paths_mode_one_alignment_object_for_every_pair(tmp_path):
    """Alignment::construct_alignment(.., with_path = true), path() and score() against _path_reference.path: a long pair, a shorter
    one, (1, 1), (1, 25) and the long pair again on ONE object, so that path_ is resized down, to nothing and up again and the
    context's pair batch is replaced and made anew."""
    import _path_reference as pr
    import _spot_path_reference as spp
    pct, pen, dim = 0.0625, PATH_SKEWED, 13
    seqs = gauss((90, 77, 33, 41, 1, 1, 25), dim, 9101)
    pairs = [(0, 1), (2, 3), (4, 5), (4, 6), (0, 1)]
    text = header_text(pct, pen, dim) + set_text(seqs) + "".join("pair %d %d\n" % p for p in pairs)
    out = run_mode("paths", text, tmp_path)
    got = []
    for x, y in pairs:
        gx, gy, n, m, score, used = out.take("pair")
        assert (int(gx), int(gy), int(n), int(m)) == (x, y, len(seqs[x]), len(seqs[y]))
        got.append((out.steps(int(used)), np.array([int(score, 16)], dtype=np.uint32).view(F)))
    out.done()
    for (x, y), (steps, score) in zip(pairs, got):
        n, m = len(seqs[x]), len(seqs[y])
        want_steps, want_score = pr.path(seqs[x], seqs[y], pr.band_from_pct(pct, max(n, m)), *pen)
        assert spp.same_steps(steps, want_steps), (x, y)
        assert same_f32(score, want_score), (x, y)
    assert len(got[0][0]) >= 90 and got[0][0][0]["op"] == pr.START and tuple(got[0][0][-1][["i", "j"]]) == (89, 76)
    assert [tuple(s) for s in got[2][0]] == [(0, 0, 0.0, pr.START)] and got[2][1][0] == 0.0        # n = m = 1: the one step
    assert len(got[3][0]) == 0 and np.isposinf(got[3][1][0])                                       # exactly one length is 1: no path
    assert spp.same_steps(got[4][0], got[0][0]) and same_f32(got[4][1], got[0][1])


def test_cross_mode_two_workers_and_a_joined_batch(oracle, apd, tmp_path):
    """AlignmentWorkers::cross and Batch::join / len / first_len: the bits of the Python mirror's cross() (the same library, the same
    kernels, the default distance mode), and the oracle at the suite's 1e-4 with identical zeros and +INF pattern."""
    from audio_pattern_discovery_amd.alignments import AlignmentWorkers, NDSequence
    from audio_pattern_discovery_amd.discovery import Discovery
    from test_gpu_cross import oracle_cross, walks
    from test_gpu_kernel_matrix import check
    pct, dim = 0.0625, 13
    a, b = walks("cpp-mirror-first", (20, 45, 33, 60, 27), dim), walks("cpp-mirror-second", (52, 24, 90, 38, 41, 29, 66), dim)
    out = run_mode("cross", header_text(pct, UNIT, dim) + set_text(a) + set_text(b), tmp_path)
    shape_fs, shape_sf = (len(a), len(b)), (len(b), len(a))
    fs, sf = out.f32("fs").reshape(shape_fs), out.f32("sf").reshape(shape_sf)
    assert out.ints("join") == [len(a) + len(b), len(a)]
    direct = out.f32("direct_fs").reshape(shape_fs), out.f32("direct_sf").reshape(shape_sf)
    assert out.ints("parts") == [len(a), len(a), len(b), len(b)]
    again = out.f32("again_fs").reshape(shape_fs), out.f32("again_sf").reshape(shape_sf)
    out.done()
    ctx = apd.Context(0)
    try:
        wa, wb = AlignmentWorkers.new([NDSequence(s) for s in a], ctx), AlignmentWorkers.new([NDSequence(s) for s in b], ctx)
        mirror = wa.cross(wb, Discovery(warping_band_percentage=pct))
        wa.close()
        wb.close()
    finally:
        ctx.close()
    for what, (g_fs, g_sf) in (("cross()", (fs, sf)), ("apd_align_cross on Batch::join", direct), ("cross() again", again)):
        check(g_fs, mirror[0], True, what + ", fs against the Python mirror")
        check(g_sf, mirror[1], True, what + ", sf against the Python mirror")
    want_fs, want_sf = oracle_cross(oracle, "cpp-mirror", a, b, dim, pct)
    check(fs, want_fs, False, "fs against the oracle")
    check(sf, want_sf, False, "sf against the oracle")


def test_spot_mode_curves_hits_and_paths(tmp_path):
    """AlignmentWorkers::spot in its four forms, apd::spot_hits and AlignmentWorkers::spot_paths against _spot_reference.spot / hits
    and _spot_path_reference.answer.  Queries of 30, 29 and 1 frames (sequences 0 .. 2), streams of 40 and 91 frames (3, 4); the long
    stream holds two noisy copies of query 0, so a threshold between their scores and the rest gives several hits."""
    import _spot_path_reference as spp
    import _spot_reference as sp
    pen, dim = SPOT_SKEWED, 13
    rng = np.random.default_rng(9103)
    queries, streams = gauss((30, 29, 1), dim, 9104), gauss((40, 91), dim, 9105)
    for at in (8, 52):
        streams[1][at:at + 30] = queries[0] + F(0.05) * rng.standard_normal((30, dim)).astype(F)
    seqs = queries + streams
    pairs = [(0, 4), (1, 3), (2, 4), (0, 3), (1, 4), (2, 3), (0, 4)]
    want = [sp.spot(seqs[x], seqs[y], *pen) for x, y in pairs]
    cost, start, best = want[0]
    scores = np.sort(sp.scores(cost, start, 30))
    threshold = F((scores[1] + scores[-1]) / 2)
    want_hits = sp.hits(cost, start, 30, threshold)
    assert len(want_hits) >= 2 and len(sp.hits(cost, start, 30, F(0.0))) == 0
    tab = spp.table(seqs[0], seqs[4], *pen)
    wrong = (int(best["end"]), int(best["start"]) + (1 if best["start"] < best["end"] else -1))
    assert spp.answer(tab, 30, *wrong)[1] == int(best["start"]) != wrong[1]
    listed = [(0, 4, 0, 0), (0, 4) + wrong, (2, 3, int(want[5][2]["end"]), int(want[5][2]["start"])),
              (1, 3, 40, int(want[1][1][39])), (0, 4, int(want_hits[0]["end"]), int(want_hits[0]["start"]))]
    pair_text = "%d %s\n" % (len(pairs), " ".join("%d %d" % p for p in pairs))
    text = (header_text(0.5, pen, dim) + set_text(queries) + set_text(streams)
            + "spot 1 1 " + pair_text + "hits 0 30 %s\n" % hx([threshold]) + "paths 1 1 0 4 %s\n" % windows_text(listed)
            + "paths 0 1 0 4 0\n" + "hits 6 30 %s\n" % hx([0.0]) + "paths 1 1 0 4 0\n" + "paths 0 0 %s\n" % windows_text(listed)
            + "spot 1 0 " + pair_text + "spot 0 1 " + pair_text + "spot 0 0 " + pair_text)
    out = run_mode("spot", text, tmp_path)

    def check_spotted(curves, what):
        bests, got_curves = out.spotted("spot")
        assert len(bests) == len(pairs) and len(got_curves) == (len(pairs) if curves else 0), what
        for p, (w_cost, w_start, w_best) in enumerate(want):
            assert sp.same_best(bests[p], w_best), (what, pairs[p])
            if curves:
                assert same_f32(got_curves[p][0], w_cost) and np.array_equal(got_curves[p][1], w_start), (what, pairs[p])

    def check_paths(windows, what):
        got = out.paths()
        assert len(got) == len(windows), what
        for g, (x, y, end, start) in zip(got, windows):
            w = spp.answer(spp.table(seqs[x], seqs[y], *pen), len(seqs[x]), end, start)
            assert same_window(g, w), (what, (x, y, end, start))
        return got

    check_spotted(True, "curves, streams")
    (count,) = out.ints("hits")
    hits = np.array([out.best() for _ in range(count)], dtype=sp.BEST)
    assert sp.same_best(hits, want_hits)
    of_hits = [(0, 4, int(h["end"]), int(h["start"])) for h in want_hits]
    got = check_paths(of_hits + listed, "one window per hit and the listed ones, streams")
    assert all(len(g[0]) > 0 and g[0][0]["op"] == spp.START for g in got[:len(of_hits)])     # a pair repeated once per hit
    none, wrong_start = got[len(of_hits)], got[len(of_hits) + 1]
    assert len(none[0]) == 0 and none[1] == 0 and np.isposinf(none[2][0])                  # {0, 0}: no window
    assert len(wrong_start[0]) == 0 and wrong_start[1] == int(best["start"])               # found_start says which start to ask with
    check_paths(of_hits, "one window per hit, one batch")
    assert out.ints("hits") == [0]
    check_paths([], "no hit: an empty window list")
    check_paths(listed, "the listed windows, one batch")
    check_spotted(True, "curves, one batch")
    check_spotted(False, "best only, streams")
    check_spotted(False, "best only, one batch")
    out.done()


def test_stream_mode_a_session_returned_by_value(apd, tmp_path):
    """AlignmentWorkers::spot_stream and every member of SpotStream against _spot_stream_reference.run and
    _spot_stream_path_reference.expected.  Queries [0, 1, 0] (30, 9 and again 30 frames), two channels, pair = channel * 3 + q.
    Pushes: a zero-length chunk on one channel, a one-frame chunk, a push of nothing at all (the curves buffer of one entry), one
    without curves; then channel 1 alone starts over at column 500, H = 24 columns are kept from there on, and 30 (channel 0) and 66
    (channel 1) more columns arrive, so both rings wrap.  Windows: traced, aged out by their end, aged out by their start, a wrong
    start, {0, 0}, an empty list, and a refused one (its end is not pushed yet) after which the session goes on.  found_start and
    history() must also be what the C ABI reports for the same session through ctypes."""
    import _spot_path_reference as spp
    import _spot_reference as sp
    import _spot_stream_path_reference as hist
    import _spot_stream_reference as sref
    from test_gpu_spot import make_batch
    from test_gpu_spot_stream_paths import HistoryStream
    pen, dim, H = SPOT_SKEWED, 3, 24
    templates, (y0, y1) = gauss((30, 9), dim, 9106), gauss((40, 91), dim, 9107)
    queries, lens = [0, 1, 0], [30, 9, 30]
    # (curves, frames of channel 0, frames of channel 1) per push; the reset and the keep come after the fourth
    sizes = [(1, 5, 0), (1, 1, 7), (1, 0, 0), (0, 4, 10), (1, 10, 30), (1, 20, 31), (1, 0, 5)]
    cuts0, cuts1 = np.cumsum([0] + [s[1] for s in sizes]), np.cumsum([0] + [s[2] for s in sizes])
    chunks = [(y0[cuts0[r]:cuts0[r + 1]], y1[cuts1[r]:cuts1[r + 1]]) for r in range(len(sizes))]
    first_column, origin0 = 500, int(cuts0[4])
    since_reset = y1[cuts1[4]:cuts1[7]]
    # the checker: per pair the pushes of its stream, channel 1 as two streams (before and after its reset)
    runs = {}
    for q, x in enumerate(queries):
        runs[(0, q)] = sref.run(templates[x], [c[0] for c in chunks], *pen)
        runs[(1, q)] = (sref.run(templates[x], [c[1] for c in chunks[:4]], *pen)
                        + sref.run(templates[x], [c[1] for c in chunks[4:]], *pen, first_column=first_column))
    tabs = {(0, x): spp.table(templates[x], y0, *pen) for x in (0, 1)}
    tabs.update({(1, x): spp.table(templates[x], since_reset, *pen) for x in (0, 1)})

    def kept_after(r):
        """[(first, last)] per channel after push r (r >= 4: the history is on)."""
        last0, last1 = int(cuts0[r + 1]), first_column + int(cuts1[r + 1] - cuts1[4])
        return [(max(origin0 + 1, last0 - H + 1), last0), (max(first_column + 1, last1 - H + 1), last1)]

    def windows_after(r):
        out = []
        for k, (first, last) in enumerate(kept_after(r)):
            fc = first_column if k else 0
            for q, x in enumerate(queries):
                starts = tabs[(k, x)][1][lens[q]]
                for end in (last, last - 3, first, first - 1, first - 9):
                    out.append((q, k, end, int(starts[end - fc]) + fc if starts[end - fc] else 0))
                found = int(starts[last - fc]) + fc
                out.append((q, k, last, [s for s in (found + 1, found - 1) if fc + 1 <= s <= last][0]))   # a wrong start
                out.append((q, k, 0, 0))
        return out

    def expected(r, window):
        q, k, end, start = window
        fc = first_column if k else 0
        whole = spp.answer(tabs[(k, queries[q])], lens[q], end - fc if end else 0, start - fc if start else 0)
        return hist.expected(whole, lens[q], fc, kept_after(r)[k], end, start)

    asked5, asked6 = windows_after(5), windows_after(6)
    wants5 = [expected(5, w) for w in asked5]
    traced = sum(len(w[0]) > 0 for w in wants5)
    by_end = sum(w[2] > 0 and w[2] < kept_after(5)[w[1]][0] for w in asked5)
    by_start = sum(len(e[0]) == 0 and e[1] == w[3] > 0 for w, e in zip(asked5, wants5))
    assert traced >= 4 and by_end >= 4 and by_start >= 2, (traced, by_end, by_start)   # before the GPU is touched
    beyond = (0, 1, kept_after(5)[1][1] + 1, kept_after(5)[1][1] + 1)

    def push_text(r):
        return "push %d %d %d\n%s\n%s\n" % (sizes[r][0], sizes[r][1], sizes[r][2], hx(chunks[r][0]), hx(chunks[r][1]))

    text = (header_text(0.5, pen, dim) + set_text(templates) + "3 0 1 0\n2\n" + "".join(push_text(r) for r in range(4))
            + "history\nreset 1 %d\nkeep %d\nhistory\n" % (first_column, H) + push_text(4) + push_text(5) + "history\n"
            + "paths %s\npaths 0\nrefusal paths %s\nhistory\n" % (windows_text(asked5), windows_text([beyond]))
            + push_text(6) + "history\npaths %s\n" % windows_text(asked6))
    out = run_mode("stream", text, tmp_path)

    def check_push(r):
        bests, curves = out.spotted("push")
        assert len(bests) == 6 and len(curves) == (6 if sizes[r][0] else 0), r
        for k in range(2):
            for q in range(3):
                w_cost, w_start, w_best = runs[(k, q)][r]
                assert sp.same_best(bests[k * 3 + q], w_best), (r, k, q)
                if sizes[r][0]:
                    g_cost, g_start = curves[k * 3 + q]
                    assert len(g_cost) == sizes[r][1 + k] and same_f32(g_cost, w_cost) and np.array_equal(g_start, w_start), (r, k, q)
        columns = out.ints("columns")
        assert columns == [int(cuts0[r + 1]), int(cuts1[r + 1]) if r < 4 else first_column + int(cuts1[r + 1] - cuts1[4])], r
        return columns

    def check_history(want):
        got = [tuple(out.ints("history")) for _ in range(2)]
        assert got == [(0,) + want[0], (1,) + want[1]]
        return [g[1:] for g in got]

    def check_paths(r, windows):
        got = out.paths()
        assert len(got) == len(windows)
        for g, w in zip(got, windows):
            assert same_window(g, expected(r, w)), (r, w)
        return got

    for r in range(4):
        check_push(r)
    check_history([(11, 10), (18, 17)])                                                 # no history: first = last + 1
    assert out.ints("columns") == [10, first_column]                                    # the reset channel restarts at first_column
    check_history([(11, 10), (first_column + 1, first_column)])
    check_push(4)
    check_push(5)
    histories = [check_history(kept_after(5))]
    assert kept_after(5) == [(17, 40), (538, 561)]
    got5 = check_paths(5, asked5)
    assert all(len(g[0]) == 0 for g, w in zip(got5, asked5) if w[2] == 0 or w[2] < kept_after(5)[w[1]][0])
    assert sum(len(g[0]) > 0 for g in got5) == traced
    assert out.ints("paths") == [0]                                                      # an empty window list
    status = out.take("error")
    assert int(status[0]) == apd.APD_ERR_INVALID_ARG
    histories.append(check_history(kept_after(5)))                                      # the refusal touched nothing
    check_push(6)
    histories.append(check_history(kept_after(6)))
    got6 = check_paths(6, asked6)
    out.done()

    # the same session through the C ABI: history and found_start
    ctx = apd.Context(0)
    try:
        batch = make_batch(ctx, templates)
        try:
            with HistoryStream(apd, ctx, batch, queries, pen, 2) as raw:
                for r in range(4):
                    raw.push(list(chunks[r]), curves=bool(sizes[r][0]))
                assert raw.reset(1, first_column) == apd.APD_OK and raw.keep(H) == apd.APD_OK
                raw.push(list(chunks[4]))
                raw.push(list(chunks[5]))
                raw_histories = [[raw.history(k) for k in range(2)]]
                _, found5, _ = raw.paths(asked5, lens)
                raw_histories.append([raw.history(k) for k in range(2)])
                raw.push(list(chunks[6]))
                raw_histories.append([raw.history(k) for k in range(2)])
                _, found6, _ = raw.paths(asked6, lens)
        finally:
            batch.close()
    finally:
        ctx.close()
    assert histories == raw_histories
    assert [g[1] for g in got5] == found5.tolist() and [g[1] for g in got6] == found6.tolist()


def test_prototypes_mode_medoids_barycenters_and_linkage(apd, tmp_path):
    """AgglomerativeClustering::medoids on the workers' own result, AlignmentWorkers::barycenters and
    AgglomerativeClustering::cross_linkage on cross()'s matrices, against _dba_reference and _linkage_reference.reference.  Sets
    listed unsorted, an empty set, a singleton, an init that is no member, a one-frame init; iterations 0 and 2; no set at all."""
    import _dba_reference as dba
    from _linkage_reference import assert_equal, reference
    pct, pen, dim = 0.25, PATH_SKEWED, 3
    a = gauss((20, 31, 26, 44, 38, 23, 50, 29, 35, 41, 27, 1), dim, 9108)
    b = gauss((33, 20, 58, 41, 25, 47, 36, 29), dim, 9109)
    medoid_sets = [[4, 2, 7], [], [5], [9, 0, 3, 1], [8, 10, 6]]
    bary_sets, init = [[4, 2, 7], [], [5], [9, 0, 3, 1], [8, 10]], [6, 0, 5, 11, 8]
    link_sets = [[5, 1, 7], [], [3], [0, 2, 6, 4]]
    bary_text = "%s %d %s\n" % (sets_text(bary_sets), len(init), " ".join(str(i) for i in init))
    text = (header_text(pct, pen, dim) + set_text(a) + set_text(b) + "medoids %s\n" % sets_text(medoid_sets)
            + "bary 0 " + bary_text + "bary 2 " + bary_text + "refusal bary 1 %s 1 0\n" % sets_text(bary_sets[:2])
            + "linkage %s\nlinkage 0\n" % sets_text(link_sets))
    out = run_mode("prototypes", text, tmp_path)
    dist = out.f32("dist").reshape(len(a), len(a))
    fs, sf = out.f32("fs").reshape(len(a), len(b)), out.f32("sf").reshape(len(b), len(a))
    assert np.all(np.diag(dist) == 0) and np.isfinite(dist[:11, :11]).all()

    want_m, want_c = dba.medoids(dist, medoid_sets)
    assert np.array_equal(out.u32("medoid"), want_m) and same_f32(out.f32("cost"), want_c)
    assert want_m[1] == dba.NONE and want_m[2] == 5 and len(set(want_m.tolist())) == 5

    for iterations in (0, 2):
        assert out.ints("bary") == [len(bary_sets)]
        flat = [out.f32("frames") for _ in bary_sets]
        assert [len(f) for f in flat] == [dim * (len(a[i]) if s else 0) for i, s in zip(init, bary_sets)], iterations
        frames = [f.reshape(-1, dim) for f in flat]
        inertia, used = out.f32("inertia").reshape(iterations, len(bary_sets)), out.u32("used").reshape(iterations, len(bary_sets))
        w_frames, w_inertia, w_used = dba.barycenters(a, bary_sets, init, pct, pen, iterations)
        assert [len(f) for f in frames] == [len(w) for w in w_frames] == [50, 0, 23, 1, 35]
        assert all(same_f32(g, w) for g, w in zip(frames, w_frames)), iterations
        assert same_f32(inertia, w_inertia) and np.array_equal(used, w_used), iterations
        if iterations == 0:                                                              # the init frames, byte for byte
            assert all(g.tobytes() == a[i].tobytes() for g, i, s in zip(frames, init, bary_sets) if s)
        else:
            assert used[0].tolist() == [3, 0, 1, 0, 2] and not np.array_equal(frames[0], a[6])
    status = out.take("error")
    assert int(status[0]) == apd.APD_ERR_INVALID_ARG

    got = out.f32("link_fs").reshape(len(a), -1), out.f32("link_sf").reshape(len(a), -1), out.u32("nearest"), out.f32("nearest_linkage")
    want = reference(fs, sf, link_sets)
    assert_equal(got, want, "four sets of the second set")
    assert np.isnan(got[0][:, 1]).all() and not np.any(got[2] == 1)
    listed = reference(fs, sf, link_sets, ascending=False)
    assert (want[0].view(np.uint32) != listed[0].view(np.uint32)).any()                  # the ascending order shows in these bits
    none = out.f32("link_fs"), out.f32("link_sf"), out.u32("nearest"), out.f32("nearest_linkage")
    assert len(none[0]) == 0 and len(none[1]) == 0 and np.all(none[2] == dba.NONE) and np.isposinf(none[3]).all() and len(none[2]) == len(a)
    out.done()
