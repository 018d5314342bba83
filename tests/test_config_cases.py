"""CPU tests of the degenerate alignment configurations of tests/_config_cases.py: the checkers agree with each other over the whole
table, survive it (no abort, no exception, no dependence on numpy's warning state), show the effects the table claims, and the
host-only entry points of the product follow them.  The GPU side is tests/test_gpu_config_edges.py.

The per-cell Python checkers (oracle/np_reference.py, tests/_path_reference.py) walk _config_cases.SLOW_PAIRS of batch A; the two
C forms are compared on every ordered pair of the batch."""
import os
import shutil
import struct
import subprocess
import warnings

import numpy as np
import pytest

import _config_cases as cc
import _path_reference as ref
from oracle import np_reference as npref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = cc.ENTRIES + [cc.ROUNDING_ENTRY]
IDS = [e.name for e in ALL]


def hexbits(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", v))[0]


def grid_lines():
    """The table as oracle_grid reads it: every entry, and every explicit band under unit penalties and under a zero one."""
    lines = ["%s %s %s P %s" % (hexbits(e.pens[0]), hexbits(e.pens[1]), hexbits(e.pens[2]), hexbits(e.pct)) for e in ALL]
    for band in cc.EXPLICIT_BANDS:
        for p in ("unit", "ins0", "all-inf"):
            pens = cc.PENS[p]
            lines.append("%s %s %s B %d" % (hexbits(pens[0]), hexbits(pens[1]), hexbits(pens[2]), 33 if band is None else band))
    return lines


def test_the_oracle_survives_the_grid_under_the_sanitizers(tmp_path):
    """oracle/apd_oracle.c and tools/fuzz/oracle_grid.c (its own main) built under AddressSanitizer + UBSan and run as a child
    process over the whole table: dense form, hash-map form and cell count on tiny pairs of lengths 1, 2, 3, 7, 20, 33 in both
    orders.  Before the band was clamped to max(n, m), a saturated percentage wrapped w to 1 and the dense rows were written out of
    bounds."""
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    exe, grid = str(tmp_path / "oracle_grid"), tmp_path / "grid.txt"
    lines = grid_lines()
    grid.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-ffp-contract=off", "-fopenmp", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "oracle"), os.path.join(ROOT, "oracle", "apd_oracle.c"),
                           os.path.join(ROOT, "tools", "fuzz", "oracle_grid.c"), "-o", exe, "-lm", "-lpthread"])
    out = subprocess.run([exe, str(grid)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "no sanitizer report" in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]
    assert "%d configurations, %d runs" % (len(lines), 36 * len(lines)) in out.stdout


def test_the_probes_that_aborted_the_interpreter_return_the_full_band_matrix(oracle):
    """oracle.align_all with pct = 1e30 / +inf on six sequences of about 20 frames, dim 5: `malloc(): corrupted top size` before the
    clamp.  Now the pct = 1.0 matrix."""
    from audio_pattern_discovery_amd import synth
    frames, offsets = synth.make_sequences(6, 20, 5, seed=3, jitter=6)
    full = oracle.align_all(frames, offsets, 1.0, 1, 1, 1)
    for pct in (1e30, float("inf"), 1e10, 1.5):
        for hashmap in (False, True):
            assert np.array_equal(oracle.align_all(frames, offsets, pct, 1, 1, 1, hashmap=hashmap), full), pct


def test_no_checker_raises_or_depends_on_the_warning_state(oracle):
    """Every band helper over every percentage and the per-cell checkers over the NaN / INF penalty sets, with numpy's floating
    point errors raised and Python's warnings turned into errors."""
    b = cc.batch("A")
    x, y = b.seqs[2], b.seqs[1]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with np.errstate(all="raise"):
            for _, pct in cc.PERCENTAGES + [("rounding", cc.PCT_ROUNDING), ("binds", cc.PCT_BINDS)]:
                for length in (1, 10, 130, 1 << 20, 1 << 40):
                    want = oracle.warping_band(pct, length)
                    assert ref.band_from_pct(pct, length) == want and npref.warping_band(pct, length) == want, (pct, length)
                    assert 0 <= want <= 2 ** 64 - 1
            assert ref.band_from_pct(float("inf"), 10) == 2 ** 64 - 1 and ref.band_from_pct(1e30, 10) == 2 ** 64 - 1
            assert ref.band_from_pct(cc.PCT_ROUNDING, 10) == 7
            for name in ("all-inf", "ins-nan", "mat-nan", "all-1", "extremes", "subnormal", "all0"):
                pens = cc.PENS[name]
                for band in (0, 2 ** 64 - 1, 2 ** 80):
                    ref.path(x, y, band, *pens)
                    npref.dtw_pair(x, y, band, *pens)
                    ref.replay(x, y, ref.path(x, y, band, *pens)[0], *pens)


@pytest.mark.parametrize("entry", ALL, ids=IDS)
def test_the_two_c_forms_agree_on_every_pair(oracle, entry):
    key = "R" if entry is cc.ROUNDING_ENTRY else "A"
    b = cc.batch(key)
    dense = cc.want_matrix(oracle, key, entry)
    sparse = oracle.align_all(b.frames, b.offsets, entry.pct, *entry.pens, workers=4, hashmap=True)
    assert cc.same_bits(dense, sparse)
    assert np.all(np.diag(dense) == 0)


@pytest.mark.parametrize("entry", ALL, ids=IDS)
def test_the_python_checkers_agree_with_the_oracle(oracle, entry):
    """Dense oracle == np_reference == the score cell of _path_reference.table == _path_reference.path's score, bit for bit (NaN
    aside), and orc_dtw_cells == the cells the table checker visits."""
    key = "R" if entry is cc.ROUNDING_ENTRY else "A"
    b = cc.batch(key)
    pairs = [(a, c) for a in range(len(b.seqs)) for c in range(len(b.seqs)) if a != c] if key == "R" else cc.SLOW_PAIRS
    want = cc.want_matrix(oracle, key, entry)
    for a, c in pairs:
        x, y = b.seqs[a], b.seqs[c]
        n, m = len(x), len(y)
        band = oracle.warping_band(entry.pct, max(n, m))
        assert ref.band_from_pct(entry.pct, max(n, m)) == band
        what = "%s pair (%d, %d)" % (entry.name, a, c)
        assert cc.same_bits([oracle.dtw_pair(x, y, band, *entry.pens)], [want[a, c]]), what
        assert cc.same_bits([npref.dtw_pair(x, y, band, *entry.pens)], [want[a, c]]), what
        sparse, branch = ref.table(x, y, band, *entry.pens)
        cell = sparse.get((n - 1, m - 1))
        with np.errstate(all="ignore"):
            score = ref.INF if cell is None else ref.F(cell / ref.F(n + m))
        assert cc.same_bits([score], [want[a, c]]), what
        assert cc.same_bits([ref.path(x, y, band, *entry.pens)[1]], [want[a, c]]), what
        assert oracle.dtw_cells(n, m, band) == len(branch), what


def off_diagonal(m):
    return m[~np.eye(len(m), dtype=bool)]


def test_claimed_effects_of_the_penalty_entries(oracle):
    """From the oracle alone: what the table says the entries are for."""
    a = cc.batch("A")
    # the one-frame sequence 0 has no score cell against a longer one ((0, m-1) and (n-1, 0) are never visited): +INF whatever
    # the penalties (alignments.rs:122); everything else is the off-diagonal the claims are about
    absent = np.zeros((len(a.seqs), len(a.seqs)), dtype=bool)
    absent[0, 1:] = absent[1:, 0] = True
    zero = cc.want_matrix(oracle, "A", cc.BY_NAME["all0/pct0.0625"])
    assert np.all(zero[~absent] == 0) and not np.signbit(zero[~absent]).any() and np.all(np.isposinf(zero[absent]))
    negzero = cc.want_matrix(oracle, "A", cc.BY_NAME["all-negzero/pct0.0625"])
    assert np.all(negzero[~absent] == 0) and np.all(np.isposinf(negzero[absent]))
    minus = off_diagonal(cc.want_matrix(oracle, "A", cc.BY_NAME["all-1/pct0.0625"]))
    # every finite score is negative except between the duplicates and the one-frame pairs whose score cell is (0, 0) itself
    assert np.all(minus[np.isfinite(minus)] <= 0) and (minus < 0).sum() > 300
    # a +INF penalty gives NaN exactly where its branch meets a zero distance: the duplicate pair under an infinite MATCH penalty
    # walks its zero diagonal (INF * 0), every other pair has no zero distance on a MATCH and is +INF or finite
    mat_inf = cc.want_matrix(oracle, "A", cc.BY_NAME["mat-inf/pct0.0625"])
    nan = np.isnan(mat_inf)
    assert nan[cc.DUP_A] and nan[cc.DUP_A[::-1]]
    d_first = ref.distances(a.seqs[cc.DUP_A[0]], a.seqs[cc.DUP_A[1]])
    assert np.all(np.diag(d_first) == 0)
    for x in range(len(a.seqs)):
        for y in range(len(a.seqs)):
            if x != y and nan[x, y]:
                assert (ref.distances(a.seqs[x], a.seqs[y]) == 0).any(), (x, y)          # no NaN without a zero distance
    all_inf = cc.want_matrix(oracle, "A", cc.BY_NAME["all-inf/pct0.0625"])
    assert np.isnan(all_inf[cc.DUP_A]) and np.isposinf(all_inf[3, 4])
    # a NaN penalty reaches every score whose path takes its branch
    assert np.isnan(off_diagonal(cc.want_matrix(oracle, "A", cc.BY_NAME["mat-nan/pct0.0625"]))).sum() > 300
    # -0.0 is 0.0 as a penalty, bit for bit in the scores
    assert cc.same_bits(cc.want_matrix(oracle, "A", cc.BY_NAME["negzero/pct0.0625"]), cc.want_matrix(oracle, "A", cc.BY_NAME["ins0/pct0.0625"]))


@pytest.mark.parametrize("pname", ["unit", "ins0", "extremes"])
def test_claimed_effects_of_the_percentage_entries(oracle, pname):
    full = cc.want_matrix(oracle, "A", cc.BY_NAME[pname + "/pct1"])
    for name, _ in cc.PCT_SATURATED:
        assert cc.same_bits(cc.want_matrix(oracle, "A", cc.BY_NAME["%s/%s" % (pname, name)]), full), name
    none = cc.want_matrix(oracle, "A", cc.BY_NAME[pname + "/pct0"])
    for name, _ in cc.PCT_VANISHING:
        assert cc.same_bits(cc.want_matrix(oracle, "A", cc.BY_NAME["%s/%s" % (pname, name)]), none), name
    binds = cc.want_matrix(oracle, "A", cc.BY_NAME[pname + "/pct0.0625"])
    assert not cc.same_bits(full, none) and not cc.same_bits(binds, none) and not cc.same_bits(binds, full)


def test_the_band_binds_for_some_pairs_and_the_gap_widens_it_for_others(oracle):
    lens = cc.batch("A").lens
    bound = [(n, m) for n in lens for m in lens if oracle.warping_band(cc.PCT_BINDS, max(n, m)) > abs(n - m) and max(n, m) > 8]
    widened = [(n, m) for n in lens for m in lens if oracle.warping_band(cc.PCT_BINDS, max(n, m)) < abs(n - m)]
    assert len(bound) >= 10 and len(widened) >= 100


def test_the_f32_rounding_percentage_is_band_7_and_band_6_would_show(oracle):
    """float32(0.7) * 10: 7.0 exactly as an f32 product (discovery.rs:40), 6.99999988 in f64.  Batch R under the rounding entry's
    penalties has scores that differ between the explicit bands 6 and 7, so a product computed in double cannot hide."""
    assert np.float32(cc.PCT_ROUNDING) * np.float32(10) == np.float32(7.0) and int(np.float64(cc.PCT_ROUNDING) * 10.0) == 6
    assert oracle.warping_band(cc.PCT_ROUNDING, 10) == 7
    b = cc.batch("R")
    want = cc.want_matrix(oracle, "R", cc.ROUNDING_ENTRY)
    changed = 0
    for x in range(len(b.seqs)):
        for y in range(len(b.seqs)):
            if x == y or max(b.lens[x], b.lens[y]) != 10:
                continue
            s7 = oracle.dtw_pair(b.seqs[x], b.seqs[y], 7, *cc.ROUNDING_ENTRY.pens)
            s6 = oracle.dtw_pair(b.seqs[x], b.seqs[y], 6, *cc.ROUNDING_ENTRY.pens)
            assert cc.same_bits([s7], [want[x, y]])
            changed += int(not cc.same_bits([s6], [s7]))
    assert changed >= 1


def test_parity_entries_have_no_score_a_relative_bound_cannot_hold(oracle):
    """An equal-penalty entry is held to 1e-4 relative only if the oracle's matrices have no non-zero score below 2^-100: a
    subnormal score under a relative bound would fail a correct kernel."""
    parity = [e for e in cc.ENTRIES if e.bound == cc.PARITY]
    assert {e.pens for e in parity} == {cc.PENS["unit"], cc.PENS["p2^60"], cc.PENS["p2^-60"]}
    for e in parity:
        for key in ("A", "B"):
            m = np.abs(cc.want_matrix(oracle, key, e))
            assert not ((m != 0) & (m < 2.0 ** -100)).any(), (e.name, key)
            assert not np.isnan(m).any()
    for e in cc.ENTRIES:
        if any(p != 0 and abs(p) < 2.0 ** -126 for p in e.pens):
            assert e.bound == cc.BITWISE and not (e.pens[0] == e.pens[1] == e.pens[2])
        assert e.bound == (cc.PARITY if (e.pens[0] == e.pens[1] == e.pens[2] and all(0 < p < float("inf") for p in e.pens)) else cc.BITWISE)


# ---- the product's host-only entry points

def test_discovery_alignment_params_saturates_like_the_oracle(oracle):
    from audio_pattern_discovery_amd.discovery import Discovery
    for _, pct in cc.PERCENTAGES + [("rounding", cc.PCT_ROUNDING), ("binds", cc.PCT_BINDS), ("one", 1.0)]:
        for n in (0, 1, 10, 130, 1 << 20, (1 << 32) - 1, 1 << 32, 1 << 40):
            got = Discovery(warping_band_percentage=pct).alignment_params(n).warping_band
            assert got == oracle.warping_band(pct, n), (pct, n)
    assert Discovery(warping_band_percentage=float("inf")).alignment_params(10).warping_band == 2 ** 64 - 1
    assert Discovery(warping_band_percentage=1e30).alignment_params(10).warping_band == 2 ** 64 - 1
    assert Discovery(warping_band_percentage=cc.PCT_ROUNDING).alignment_params(10).warping_band == 7
    p = Discovery(warping_band_percentage=0.5, insertion_penalty=float("inf"), deletion_penalty=-0.0, match_penalty=1e-44).alignment_params(8)
    assert (p.insertion_penalty, p.warping_band) == (float("inf"), 4) and np.signbit(p.deletion_penalty) and p.match_penalty == float(np.float32(1e-44))


@pytest.mark.parametrize("key", ["A", "R"])
def test_align_work_counts_the_oracles_cells_over_the_percentage_list(oracle, key):
    """apd_align_work sizes its bands with host_band_from_pct, the function the tile plan and the LDS sizes use: its cell count
    equals the oracle's for every percentage -- the float32(0.7) x 10 case of batch R included, where a product in double gives
    band 6 and fewer cells.  An explicit band never reaches apd_align_work (it takes an apd_align_config): band_from_params'
    clamp to 0xFFFFFFF0 is observed on the GPU instead, through apd_align_pair (tests/test_gpu_config_edges.py)."""
    from audio_pattern_discovery_amd import _lib
    from audio_pattern_discovery_amd.alignments import align_work
    b = cc.batch(key)
    n_seq = len(b.seqs)
    for _, pct in cc.PERCENTAGES + [("rounding", cc.PCT_ROUNDING), ("binds", cc.PCT_BINDS), ("one", 1.0)]:
        pairs, cells, _ = align_work(b.offsets, b.dim, _lib.AlignConfig(pct, 0.0, float("nan"), -1.0))
        want = sum(oracle.dtw_cells(b.lens[i], b.lens[j], oracle.warping_band(pct, max(b.lens[i], b.lens[j])))
                   for i in range(n_seq) for j in range(n_seq) if i != j)
        assert (pairs, cells) == (n_seq * (n_seq - 1), want), pct
    if key == "R":
        c7 = align_work(b.offsets, b.dim, _lib.AlignConfig(cc.PCT_ROUNDING, 1, 1, 1))[1]
        six = sum(oracle.dtw_cells(b.lens[i], b.lens[j], 6 if max(b.lens[i], b.lens[j]) == 10 else oracle.warping_band(cc.PCT_ROUNDING, max(b.lens[i], b.lens[j])))
                  for i in range(n_seq) for j in range(n_seq) if i != j)
        assert c7 > six                                              # the count tells band 7 from band 6
