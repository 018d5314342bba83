"""The header parser behind tests/test_gpu_kernel_matrix.py, without a GPU: a refactor of csrc/apd_internal.h that the parser no
longer reads, or a clamp that moved away from the Python mirror, fails here and not first on the GPU box."""
import re

import pytest

import _kernel_table as kt


def test_every_family_and_the_kernel_dims_parse():
    geoms, dims = kt.parse_table()
    assert set(geoms) == set(kt.FAMILIES)
    for fam, lst in geoms.items():
        assert lst, "%s: %s parsed to an empty list" % (kt.HEADER, kt.FAMILIES[fam][0])
        assert len(set(lst)) == len(lst), "%s lists a geometry twice" % kt.FAMILIES[fam][0]
        assert all(a > 0 and b > 0 for a, b in lst)
    assert dims and dims == sorted(set(dims)), dims         # kernel_dim() takes the first one >= d: ascending
    have, dropped = kt.pairs((geoms, dims))
    assert len(have) + len(dropped) == sum(len(v) for v in geoms.values()) * len(dims)
    for fam in kt.FAMILIES:
        assert any(p[0] == fam for p in have), "no %s kernel at any dimension" % fam
    # every listed geometry exists at some dimension: an entry beyond every clamp would be dead text in the header
    assert {p[:3] for p in have} == {(fam, a, b) for fam, lst in geoms.items() for a, b in lst}


def test_every_entry_round_trips_through_its_integer_code():
    geoms, _ = kt.parse_table()
    codes = {}
    for fam, lst in geoms.items():
        for a, b in lst:
            assert a < 100 and b < 100, (fam, a, b)           # two decimal digits each (KernelGeom::encode)
            code = kt.encode(fam, a, b)
            assert kt.decode(code) == (fam, a, b), (fam, a, b, code)
            assert code not in codes, "%d names both %r and %r" % (code, codes.get(code), (fam, a, b))
            codes[code] = (fam, a, b)
    for code in (0, 1, 99, -5, 50000, 123456):              # "any other code decodes to Generic"
        assert kt.decode(code) is None


@pytest.mark.parametrize("name", kt.CLAMPS)
def test_the_clamp_mirror_agrees_with_the_header_expression(name):
    text = kt.header_text()
    _, expr, line = kt.clamp_source(text, name)
    mirror = getattr(kt, name)
    _, dims = kt.parse_table(text)
    for d in sorted(set(range(1, 65)) | set(dims)):
        want = kt.eval_clamp(text, name, d)
        assert mirror(d) == want, "%s:%d: %s(%d) is %d by the header (%s), %d by tests/_kernel_table.py" % (
            kt.HEADER, line, name, d, want, expr, mirror(d))


def test_the_clamp_reader_reads_what_it_claims_and_refuses_the_rest():
    text = ("constexpr int max_cells_per_lane(uint32_t d) { return d < 4 ? 1 : (d <= 8 ? 2 : 3); }\n"
            "constexpr int max_strip_columns(uint32_t d) { return d <= 2 ? 7 : max_cells_per_lane(d); }\n")
    assert [kt.eval_clamp(text, "max_cells_per_lane", d) for d in (3, 4, 8, 9)] == [1, 2, 2, 3]
    assert [kt.eval_clamp(text, "max_strip_columns", d) for d in (2, 3, 9)] == [7, 1, 3]
    with pytest.raises(ValueError, match="max_cells_per_lane"):
        kt.eval_clamp("constexpr int max_cells_per_lane(uint32_t d) { return d * 2; }", "max_cells_per_lane", 3)
    with pytest.raises(ValueError, match="max_strip_columns"):
        kt.eval_clamp(text.splitlines()[0], "max_strip_columns", 3)


def test_plan_lines_are_read_per_geometry():
    err = ("[apd] rank 0/1: geometry 1609: 2 tiles, w_max 70, n_max 304\nnoise\n"
           "[apd] rank 0/1: geometry 0: 1 tiles, w_max 9, n_max 30\n[apd] rank 1/2: geometry 1609: 3 tiles, w_max 70, n_max 304\n")
    assert kt.read_plan(err) == {1609: 5, 0: 1}
    assert kt.read_plan("") == {}


def test_default_tau_and_hybrid_live_at_hand_values():
    """What tests/test_gpu_tau_gate.py builds its case list and its restore value from."""
    assert kt.default_tau() == 0.015625
    assert kt.default_tau("struct apd_context {\n    float tau = 1.0f / 32.0f;   // threshold\n};") == 0.03125
    with pytest.raises(ValueError, match="tau"):
        kt.default_tau("float tau;")
    assert [kt.hybrid_live("systolic", d) for d in (5, 8, 10, 26)] == [False, True, True, True]
    assert [kt.hybrid_live("shared", d) for d in (5, 8, 13)] == [False, True, True]
    for fam in ("wide", "strip", "banded"):
        assert [kt.hybrid_live(fam, d) for d in (8, 10, 13, 26)] == [False, True, True, True], fam
    for fam in kt.FAMILIES:
        assert not kt.hybrid_live(fam, 13, (0.7, 0.7, 0.7)) and not kt.hybrid_live(fam, 13, (0.6, 1.3, 1.0))
        assert not kt.hybrid_live(fam, 13, strict=True)
    # the two thresholds are launch_align's: the mirror is compared with the line it mirrors
    src = open(kt.HEADER.replace("apd_internal.h", "dtw_generic.hip")).read()
    m = re.search(r"part\.hybrid\s*=\s*L\.hybrid\s*&&\s*\((.*?)\);", src)
    assert m is not None, "launch_align no longer has 'part.hybrid = L.hybrid && (...)'"
    assert re.sub(r"\s+", " ", m.group(1)) == ("g.family == KernelGeom::Systolic || g.family == KernelGeom::SharedColumns ? "
                                                "L.dim >= 8 && !L.strict : L.dim >= 10 && L.band.mat == 1.0f")


# ---- the spotting kernels (tests/test_gpu_spot_matrix.py)

def test_the_spot_register_rows_parse():
    assert kt.parse_spot_register_rows() >= 1
    assert kt.parse_spot_register_rows("constexpr uint32_t kSpotRegisterRows = 7;     // rows") == 7
    with pytest.raises(ValueError, match="kSpotRegisterRows"):
        kt.parse_spot_register_rows("constexpr int kSpotRows = 4;")


def test_the_spot_mirror_at_hand_values():
    dims = [8, 10, 13, 16, 20, 26]
    assert [kt.kernel_dim(d, dims) for d in (1, 5, 8, 9, 27)] == [8, 8, 8, 10, 27]
    assert [kt.spot_rows_per_lane(n) for n in (1, 64, 65, 256, 257)] == [1, 1, 2, 4, 5]
    assert [kt.spot_row_class(8, n, dims, 4) for n in (64, 65, 256, 257)] == [1, 2, 4, 0]
    assert [kt.spot_row_class(27, n, dims, 4) for n in (64, 65, 256, 257)] == [0, 0, 0, 0]      # no kernel dimension: LDS whatever R
    assert [kt.spot_row_class(kt.kernel_dim(d, dims), 65, dims, 4) for d in (1, 5, 8, 9, 27)] == [2, 2, 2, 2, 0]
    assert kt.spot_row_class(13, 257, dims, 5) == 5 and kt.spot_row_class(13, 65, dims, 1) == 0
    # (lane, row of the lane) of query row n: spot_sweep's lane_n = (n - 1) / R, r_n = (n - 1) - lane_n * R
    assert [kt.spot_row_n(n) for n in (1, 64, 65, 193, 222, 231, 256, 257)] == [(0, 0), (63, 0), (32, 0), (48, 0), (55, 1), (57, 2), (63, 3), (51, 1)]
    # the header this tree has: the mirror's defaults read it
    assert kt.kernel_dim(1) == min(kt.parse_dims(kt.header_text())) and kt.spot_row_class(kt.kernel_dim(1), 1) == 1


def test_spot_kernels_are_every_row_class_at_every_dimension_and_the_any_dimension_one():
    text = "constexpr int kKernelDims[] = {4, 6};\nconstexpr uint32_t kSpotRegisterRows = 2;\n"
    assert kt.spot_kernels(text) == [(1, 4), (2, 4), (0, 4), (1, 6), (2, 6), (0, 6), (0, 0)]
    kernels = kt.spot_kernels()
    _, dims = kt.parse_table()
    assert len(kernels) == len(set(kernels)) == len(dims) * (kt.parse_spot_register_rows() + 1) + 1


def test_spot_plan_lines_are_read_per_kernel_and_leave_the_tile_plan_alone():
    old = "[apd] rank 0/1: geometry 1609: 2 tiles, w_max 70, n_max 304\n"
    err = (old + "[apd] spot sweep kernel <2, 13>: 5 pairs\nnoise\n[apd] spot record kernel <0, 0>: 3 pairs, r_max 6, lds 3072 bytes\n"
           "[apd] spot sweep kernel <2, 13>: 1 pairs\n[apd] spot sweep kernel <0, 26>: 2 pairs, r_max 129, lds 66048 bytes\n")
    assert kt.read_spot_plan(err) == {("sweep", 2, 13): 6, ("record", 0, 0): 3, ("sweep", 0, 26): 2}
    launches = kt.read_spot_launches(err)
    assert [(v["kind"], v["rt"], v["d"], v["pairs"], v["r_max"], v["lds"]) for v in launches] == [
        ("sweep", 2, 13, 5, None, None), ("record", 0, 0, 3, 6, 3072), ("sweep", 2, 13, 1, None, None), ("sweep", 0, 26, 2, 129, 66048)]
    assert kt.read_plan(err) == {1609: 2}                     # the tile-plan reader sees what it saw before
    assert kt.read_spot_plan(old) == {} and kt.read_spot_plan("") == {}


def test_the_spot_matrix_cases_cover_every_kernel_exactly():
    import _spot_matrix as sm
    rows, dims = kt.parse_spot_register_rows(), kt.parse_dims(kt.header_text())
    kernels = sm.register_kernels()
    any_dims = sm.any_dimensions(dims)
    covered = [sm.register_case(*k).kernel for k in kernels] + sorted({sm.any_case(d).kernel for d in any_dims})
    for kind in kt.SPOT_KINDS:                                # the sweep and the recording sweep run the same cases
        assert sorted((kind,) + k for k in covered) == sorted((kind,) + k for k in kt.spot_kernels())
    assert len(covered) == len(dims) * (rows + 1) + 1
    for rt, d in kernels:                                     # each case reaches its own kernel and no other
        case = sm.register_case(rt, d)
        pairs = case.unit_pairs + case.skewed_pairs + case.gate_pairs
        assert {kt.spot_row_class(kt.kernel_dim(case.dim), case.lengths[x]) for x, _ in pairs} == {rt} and kt.kernel_dim(case.dim) == d
        assert len(case.gate_pairs) == (3 if rt else 0)
    for rt in range(1, rows + 1):
        lengths = sm.query_lengths(rt, rows)
        assert lengths[0] == 64 * (rt - 1) + 1 and lengths[-1] == 64 * rt
        assert {kt.spot_row_n(n)[1] for n in lengths} == set(range(rt)), lengths
    assert sm.query_lengths(4, 4) == [193, 222, 231, 256]
    assert [kt.spot_rows_per_lane(n) for n in sm.query_lengths(0, rows)] == [rows + 1, rows + 2]
    assert {d % 4 for d in any_dims[:4]} == {0, 1, 2, 3} and min(any_dims) > max(dims)      # the squared-norm slot in each float4 component
    assert all(kt.kernel_dim(d) == d and kt.spot_row_class(d, 1) == 0 for d in any_dims)
    far = sm.any_case(any_dims[-1])
    assert sorted({kt.spot_rows_per_lane(far.lengths[x]) for x, _ in far.unit_pairs}) == [1, rows + 2]
