"""GPU tests of the UPGMA merge loop's DEFRAGMENTATION path (clustering.hip: upgma_defrag_offsets_kernel, upgma_defrag_lists_kernel,
upgma_permute_kernel and the host's rotation of the working copies) and of the merge-loop variants crossed with it.

A defragmentation re-lays out the working copies of the distance matrix so that the members of every live cluster are neighbours; which
elements a linkage adds, and in which order, does not change -- only where they lie.  That claim is exact, so every check here is exact:
op records (ids, kinds, linkage bits as uint32), roots and threshold bits equal to the cached-linkage CPU oracle, and equal across
variants.  Whether a defragmentation runs at all depends on a work criterion, so every case that claims one reads the library's own
count from its APD_DEBUG_UPGMA summary line and asserts it.

Switches (read at every apd_clustering call): APD_UPGMA_DEFRAG = least number of merges between two defragmentations (0: never;
default 128 for n >= 2048, off below), APD_UPGMA_DEFRAG_ALWAYS (by presence) = skip the work criterion."""
import ctypes as C
import os
import re
from functools import lru_cache

import numpy as np
import pytest

from audio_pattern_discovery_amd import synth

pytestmark = pytest.mark.gpu

FORCED = {"APD_UPGMA_DEFRAG": "64", "APD_UPGMA_DEFRAG_ALWAYS": "1"}     # after every 64-merge batch, whatever the work
DEFAULT = {"APD_UPGMA_DEFRAG": None, "APD_UPGMA_DEFRAG_ALWAYS": None}
OFF = {"APD_UPGMA_DEFRAG": "0", "APD_UPGMA_DEFRAG_ALWAYS": None}
SWITCHES = ("APD_UPGMA_DEFRAG", "APD_UPGMA_DEFRAG_ALWAYS", "APD_UPGMA_TWO_LAUNCH", "APD_UPGMA_SHORT_CHAIN", "APD_UPGMA_SEGMENT_BLOCKS",
            "APD_UPGMA_NO_GRAPH", "APD_DEBUG_UPGMA_TIMING")
NAMES = {"Sequence2Sequence": 0, "Sequence2Cluster": 1, "Cluster2Sequence": 2, "Cluster2Cluster": 3}
SUMMARY = re.compile(r"\[apd\] upgma: (\d+) defragmentations")


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    """Every test starts from the library's defaults, with the per-call summary line on."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("APD_DEBUG_UPGMA", "1")
    return monkeypatch


def use(monkeypatch, settings):
    for name, value in settings.items():
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


@lru_cache(maxsize=4)
def matrix(n, kind):
    d = synth.make_distance_matrix(n, kind, seed=n + len(kind))
    d.setflags(write=False)
    return d


_want = {}


def oracle_result(oracle, n, kind, perc):
    """(records, roots, threshold bits) of the fast oracle, computed once per matrix for the whole module."""
    key = (n, kind, perc)
    if key not in _want:
        ops, roots, thr = oracle.clustering(matrix(n, kind), n, perc, fast=True)
        rec = np.array([(o["merge_i"], o["merge_j"], o["into"], NAMES[o["operation"]], int(np.float32(o["distance"]).view(np.uint32)))
                        for o in ops], dtype=np.int64).reshape(-1, 5)
        _want[key] = (rec, sorted(roots), int(np.float32(thr).view(np.uint32)))
    return _want[key]


def defrag_count(capfd):
    """The count of the summary line apd_clustering printed to fd 2 (exactly one line per call)."""
    found = SUMMARY.findall(capfd.readouterr().err)
    assert len(found) == 1, "expected one '[apd] upgma: N defragmentations' line, got %d" % len(found)
    return int(found[0])


def run_host(ctx, capfd, d, n, perc):
    """apd_clustering on a host matrix -> ((records, roots, threshold bits), defragmentations)."""
    from audio_pattern_discovery_amd.clustering import AgglomerativeClustering
    capfd.readouterr()
    ops, roots, thr = AgglomerativeClustering.clustering(d, n, perc, ctx, return_threshold=True)
    rec = np.array([(o.merge_i, o.merge_j, o.into, int(o.operation), int(np.float32(o.distance).view(np.uint32))) for o in ops],
                   dtype=np.int64).reshape(-1, 5)
    return (rec, sorted(roots), int(np.float32(thr).view(np.uint32))), defrag_count(capfd)


def run_device(apd, ctx, capfd, buf, n, perc):
    """apd_clustering on a device-resident matrix (distances_on_device = 1), same return as run_host."""
    capfd.readouterr()
    ops = (apd.ClusterOp * n)()
    roots = np.zeros(n, dtype=np.uint32)
    n_ops, n_roots, thr = C.c_uint32(0), C.c_uint32(0), C.c_float(0)
    apd.check(apd.lib().apd_clustering(ctx.handle, buf.at(), 1, n, perc, ops, C.byref(n_ops), roots.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       C.byref(n_roots), C.byref(thr)), ctx.handle)
    rec = np.array([(ops[k].merge_i, ops[k].merge_j, ops[k].into, ops[k].operation, int(np.float32(ops[k].distance).view(np.uint32)))
                    for k in range(n_ops.value)], dtype=np.int64).reshape(-1, 5)
    return (rec, roots[:n_roots.value].tolist(), int(np.float32(thr.value).view(np.uint32))), defrag_count(capfd)


def assert_same(got, want, what):
    """Bitwise equality of two results: op records (merge_i, merge_j, into, kind, linkage bits), roots, threshold bits."""
    g, w = got[0], want[0]
    k = min(len(g), len(w))
    bad = np.nonzero((g[:k] != w[:k]).any(axis=1))[0]
    assert bad.size == 0, "%s: first differing merge %d of %d: got %s want %s (merge_i, merge_j, into, kind, linkage bits)" % (
        what, bad[0], len(w), g[bad[0]].tolist(), w[bad[0]].tolist())
    assert len(g) == len(w), "%s: %d merges, want %d" % (what, len(g), len(w))
    assert got[1] == want[1], "%s: roots differ" % what
    assert got[2] == want[2], "%s: threshold bits %#x, want %#x" % (what, got[2], want[2])


# (n, kind, percentile, least defragmentations under the DEFAULT criterion).  Forced, every shape runs >= 4 full batches (>= 3
# defragmentations).  300 / 700: below the default's n limit (the env lifts it); 1201: n not a multiple of 4 or 32, > 1024 live clusters
# at the first defragmentation (the offsets kernel's carry); 2049: more rows than permute workgroups (a workgroup stages a second row);
# 3000 "big" / 4096 "chain" (clusters growing one member at a time, the cfg 5 proxy): the default criterion fires.
SHAPES = [(300, "ties", 0.6, 0), (700, "nan", 0.5, 0), (1201, "points", 0.05, 0), (2049, "big", 0.3, 1), (3000, "big", 0.3, 1),
          (4099, "inf", 0.95, 1), (4500, "ties", 0.5, 0), (4096, "chain", 0.05, 1)]


@pytest.mark.parametrize("n,kind,perc,default_min", SHAPES)
def test_defrag_forced_default_and_off_match_fast_oracle(ctx, oracle, capfd, switches, n, kind, perc, default_min):
    want = oracle_result(oracle, n, kind, perc)
    assert len(want[0]) >= 4 * 64, "too few merges for three forced defragmentations"
    d = matrix(n, kind)
    counts = {}
    for name, settings in (("forced", FORCED), ("default", DEFAULT), ("off", OFF)):
        use(switches, settings)
        got, counts[name] = run_host(ctx, capfd, d, n, perc)
        assert_same(got, want, "%s vs oracle" % name)
    print("n=%d %s: defragmentations forced %d, default %d, off %d" % (n, kind, counts["forced"], counts["default"], counts["off"]))
    assert counts["forced"] >= 3
    assert counts["default"] >= default_min
    if n < 2048:
        assert counts["default"] == 0                               # default: never below n = 2048
    assert counts["off"] == 0


VARIANTS = [{"APD_UPGMA_TWO_LAUNCH": "0"},                           # always [select, chain, segment]
            {"APD_UPGMA_TWO_LAUNCH": "2"},                           # always [select, chain]: every long chain walked whole
            {"APD_UPGMA_SHORT_CHAIN": "64"},                         # chains > 64 elements: segment / commit path through phys / ppool
            {"APD_UPGMA_SEGMENT_BLOCKS": "64"},                      # few segment workgroups: grid-stride over the items
            {"APD_UPGMA_NO_GRAPH": "1"}]                             # plain launches instead of graph replay


@pytest.mark.parametrize("n,kind,perc", [(700, "big", 0.9), (2049, "big", 0.3)])
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()))
def test_forced_defrag_crossed_with_merge_loop_variants(ctx, oracle, capfd, switches, variant, n, kind, perc):
    d = matrix(n, kind)
    use(switches, FORCED)
    base, nd = run_host(ctx, capfd, d, n, perc)
    assert nd >= 3
    assert_same(base, oracle_result(oracle, n, kind, perc), "forced defragmentation vs oracle")
    use(switches, variant)
    got, nd = run_host(ctx, capfd, d, n, perc)
    assert nd >= 3
    assert_same(got, base, "forced defragmentation + %s vs forced defragmentation" % variant)


@pytest.mark.parametrize("n,kind,perc", [(2049, "big", 0.3), (4096, "chain", 0.05)])
def test_forced_defrag_repeats_on_one_context(ctx, capfd, switches, n, kind, perc):
    """The same call twice on one context: a race in permute, lists or the buffer rotation would show as a difference."""
    d = matrix(n, kind)
    use(switches, FORCED)
    first, nd1 = run_host(ctx, capfd, d, n, perc)
    second, nd2 = run_host(ctx, capfd, d, n, perc)
    assert nd1 >= 3 and nd2 == nd1
    assert_same(second, first, "second forced run vs first")


@pytest.mark.parametrize("n,kind,perc", [(2049, "big", 0.3), (2049, "ties", 0.5)])
def test_forced_defrag_on_device_resident_matrix(apd, ctx, oracle, capfd, switches, n, kind, perc):
    """distances_on_device = 1: the first defragmentation reads the caller's buffer, which must never be written (the permuted copies
    rotate through the library's own buffers); results equal the host-input call and the oracle, twice on the same buffer."""
    d = matrix(n, kind)
    want = oracle_result(oracle, n, kind, perc)
    buf = ctx.upload(np.ascontiguousarray(d))
    try:
        use(switches, FORCED)
        got, nd = run_device(apd, ctx, capfd, buf, n, perc)
        after = buf.to_numpy(np.uint32)
        assert np.array_equal(after, d.view(np.uint32).ravel()), "the caller's device matrix was written"
        assert nd >= 3
        assert_same(got, want, "device input vs oracle")
        host, _ = run_host(ctx, capfd, d, n, perc)
        assert_same(got, host, "device input vs host input")
        again, nd2 = run_device(apd, ctx, capfd, buf, n, perc)
        assert np.array_equal(buf.to_numpy(np.uint32), after), "the caller's device matrix was written by the second call"
        assert nd2 == nd
        assert_same(again, got, "second device-input call vs first")
    finally:
        buf.free()


@pytest.mark.parametrize("n,min_free_gb", [(16500, 3), (32800, 12)])
def test_large_n_defrag_matches_no_defrag(ctx, capfd, switches, n, min_free_gb):
    """Sizes the oracle cannot reach in a test: device against device.  n = 16500 has > 16384 live clusters at the first
    defragmentation (the lists kernel's grid-stride loop); n = 32800 rows no longer fit in LDS (the unstaged permute branch).  The
    defragmentation-free path is oracle-checked at n = 16384 in tests/test_gpu_clustering.py."""
    try:
        avail = os.sysconf("SC_AVPHYS_PAGES") * os.sysconf("SC_PAGE_SIZE")
    except (ValueError, OSError):
        avail = 0
    if avail < min_free_gb * (1 << 30):
        pytest.skip("needs ~%d GB of free host memory for the matrix" % min_free_gb)
    d = synth.make_distance_matrix(n, "uniform", seed=n + len("uniform"))
    use(switches, OFF)
    off, nd_off = run_host(ctx, capfd, d, n, 0.02)
    use(switches, FORCED)
    forced, nd_forced = run_host(ctx, capfd, d, n, 0.02)
    print("n=%d: %d merges, %d forced defragmentations" % (n, len(off[0]), nd_forced))
    assert nd_off == 0 and nd_forced >= 3
    assert len(off[0]) > 1000
    assert_same(forced, off, "forced defragmentation vs none")
