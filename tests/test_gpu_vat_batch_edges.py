"""The VAT kernels (csrc/vat.hip) at the edges tests/test_gpu_vat_batch.py leaves out: every case of
tests/_vat_batch_cases.py -- NaN stretches on the scan's wavefront and step edges, recordings that emit as many ranges as the device
buffer holds, the percentile's index on the last classified variance, random frames at the lengths and widths where the kernels
change path -- through apd_interesting_ranges_batch in the host and the device form, in order and reversed, against the integer
model (exact cases) or the C oracle (float cases), by list equality; capacities that cut inside a wavefront's emits; min_len at and
above 2^32; apd_slice_samples at every output alignment.  tests/test_vat_batch_cases.py shows on the CPU that the cases are what
their names say."""
import numpy as np
import pytest

import _companion_cases as cc
import _vat_batch_cases as cases
from _vat_batch_calls import SENTINEL, batch_call, batch_result, gather_shifted, ramps, single_result

pytestmark = pytest.mark.gpu
FORMS = ("host", "device")


@pytest.fixture(scope="module")
def ctx(apd):
    c = apd.Context(0)
    yield c
    c.close()


def assert_every_way(apd, ctx, c, want):
    """Host and device form, in order and reversed: a recording's answer depends neither on where the frames lie nor on its neighbours."""
    for form in FORMS:
        assert batch_result(apd, ctx, c.recordings, c.k, c.perc, c.min_len, form) == want, form
        assert batch_result(apd, ctx, c.recordings[::-1], c.k, c.perc, c.min_len, form) == want[::-1], (form, "reversed")


# ------------------------------------------------------------------------------------------------ exact cases

@pytest.mark.parametrize("name", cases.names("stretch") + cases.names("verdict"))
def test_hole_cases_equal_the_model_and_the_single_call(ctx, apd, name):
    """NaN stretches on the scan's edges and the verdict boundary: the batch equals the integer model, and so does every recording
    alone through the single call, a batch of one (its workgroup size then follows that recording's own length)."""
    entry = cases.get(name)
    c, want = entry.case, entry.expected()
    assert_every_way(apd, ctx, c, want)
    assert [single_result(apd, ctx, f, c.k, c.perc, c.min_len) for f in c.recordings] == want


@pytest.mark.parametrize("name", cases.names("dense"))
def test_dense_cases_equal_the_model(ctx, apd, name):
    entry = cases.get(name)
    assert_every_way(apd, ctx, entry.case, entry.expected())


@pytest.mark.parametrize("name", [n for n in cases.names("dense") if not n.startswith("dense but")])
def test_dense_cases_under_capacities_that_cut_inside_a_wavefront(ctx, apd, name):
    """The exact total (which is also the size of the device buffer), one less, 33 less, one past the first recording: the written
    prefix is the answer's, the rest of the caller's array is untouched, range_off reports every range."""
    entry = cases.get(name)
    c, want = entry.case, entry.expected()
    flat = np.array([v for rec in want for pair in rec for v in pair], dtype=np.uint64)
    want_off = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.uint64)
    total = int(want_off[-1])
    assert total == sum(len(f) // (c.min_len + 2) for f in c.recordings) and total - 33 > len(want[0]) + 1
    for form in FORMS:
        for cap in (total, total - 1, total - 33, len(want[0]) + 1):
            rc, range_off, ranges, status = batch_call(apd, ctx, c.recordings, c.k, c.perc, c.min_len, form, capacity=cap)
            assert rc == apd.APD_OK and np.array_equal(range_off, want_off) and np.all(status == apd.APD_OK), (form, cap)
            assert np.array_equal(ranges[:2 * cap], flat[:2 * cap]) and np.all(ranges[2 * cap:] == SENTINEL), (form, cap)


@pytest.mark.parametrize("min_len", [2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1])
def test_min_len_at_and_above_two_to_the_32(ctx, apd, min_len):
    """No run of a 64- or 500-frame recording is that long: no ranges, an all-zero range_off, APD_OK, nothing written."""
    a_list = [list(cc.KAT_A), list(cc.random_integer_a()), list(cc.KAT_A)[::-1]]
    recs = [cc.alternating(a, 4) for a in a_list]
    assert all(cc.integer_ranges(a, cc.KAT_K, cases.index_of(len(a), cc.KAT_PERC), cc.KAT_MIN_LEN)[0] for a in a_list)   # ranges at a small min_len
    for form in FORMS:
        rc, range_off, ranges, status = batch_call(apd, ctx, recs, cc.KAT_K, cc.KAT_PERC, min_len, form)
        assert rc == apd.APD_OK and np.all(range_off == 0) and np.all(status == apd.APD_OK) and np.all(ranges == SENTINEL), form


# ------------------------------------------------------------------------------------------------ float cases

@pytest.mark.parametrize("name", cases.names("float"))
def test_float_cases_equal_the_oracle(ctx, apd, oracle, name):
    c = cases.get(name).case
    want = [oracle.interesting_ranges(f, c.k, c.perc, c.min_len) for f in c.recordings]
    assert any(want)
    assert_every_way(apd, ctx, c, want)


# ------------------------------------------------------------------------------------------------ the gather's head

GATHER_LENGTHS = (5003, 801, 60)
GATHER_RANGES = {                                                   # fft_step 1: a range is its samples
    "1 sample": [[(10, 11)], [], []],
    "3 samples": [[(10, 13)], [], []],
    "3 samples, three slices, one empty": [[(3, 4), (4, 4)], [(0, 2)], []],
    "7 samples, two slices": [[(0, 3)], [(5, 9)], []],
    "8 samples": [[(100, 108)], [], []],
    "9 samples, two slices": [[(100, 104)], [(0, 5)], []],
    "4099 samples": [[(1, 2001), (2500, 4500)], [(700, 799)], []],
    "a group over three slices, two of them empty": [[(0, 5)], [(7, 7), (9, 9), (9, 20)], []],
}
GATHER_TOTALS = (1, 3, 3, 7, 8, 9, 4099, 16)


@pytest.mark.parametrize("out_shift", range(0, 16, 2))
def test_gather_at_every_output_alignment(ctx, apd, out_shift):
    """The output 0 .. 14 bytes past a 16-byte boundary (heads of 0, 7, 6, .. 1 samples), the samples 0, 2 and 8 bytes past one;
    totals below the head (work-item 0 owns everything), of one group, and of many.  The whole output buffer is compared: the
    sentinel in front of the first sample and behind the last one stays."""
    recs = ramps(GATHER_LENGTHS)
    head = ((16 - out_shift) & 15) // 2
    for (what, ranges), want_total in zip(GATHER_RANGES.items(), GATHER_TOTALS):
        want = np.concatenate([recs[s][a:b] for s in range(len(recs)) for a, b in ranges[s]])
        assert len(want) == want_total
        for in_shift in (0, 2, 8):
            rc, whole, total = gather_shifted(apd, ctx, recs, ranges, 1, out_shift, in_shift)
            assert rc == apd.APD_OK and total == want_total, (what, in_shift)
            expect = np.full(len(whole), 0x5A5A, np.int16)
            expect[out_shift // 2:out_shift // 2 + total] = want
            assert np.array_equal(whole, expect), (what, in_shift, head)
    assert any(t < head for t in GATHER_TOTALS) == (head > 1)
