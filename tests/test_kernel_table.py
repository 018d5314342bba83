"""The header parser behind tests/test_gpu_kernel_matrix.py, without a GPU: a refactor of csrc/apd_internal.h that the parser no
longer reads, or a clamp that moved away from the Python mirror, fails here and not first on the GPU box."""
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
