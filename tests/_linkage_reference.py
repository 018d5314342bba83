"""Checker for apd_cross_linkage (include/apd.h): TEST INFRASTRUCTURE, no GPU, no code shared with the product.

The reference's average linkage (clustering.rs:153-170) of every first-set sequence to sets of the second, and merge()'s choice
among them (clustering.rs:178-187), as a sequential numpy-f32 loop; and the same loop with the first-set sequences as one array
operation, for first sets and set lists too large for the scalar loop (tests/test_linkage_reference.py shows the two equal)."""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF


def reference(fs, sf, sets, ascending=True):
    """(link_fs, link_sf, nearest, nearest_linkage): one rounded f32 add per member, ascending sequence number (or, to show that the
    order matters, the listed order), then one division; the scan keeps a value only if strictly below the best so far."""
    n1 = fs.shape[0]
    link_fs, link_sf = np.zeros((n1, len(sets)), F), np.zeros((n1, len(sets)), F)
    with np.errstate(all="ignore"):
        for k, s in enumerate(sets):
            members = sorted(s) if ascending else list(s)
            for q in range(n1):
                a = b = F(0.0)
                for y in members:
                    a = F(a + fs[q, y])
                    b = F(b + sf[y, q])
                link_fs[q, k] = a / F(F(1.0) * F(len(members)))
                link_sf[q, k] = b / F(F(len(members)) * F(1.0))
    nearest, best = np.full(n1, NONE, np.uint32), np.full(n1, np.inf, F)
    for q in range(n1):
        for k in range(len(sets)):
            for v in (link_fs[q, k], link_sf[q, k]):
                if v < best[q]:
                    best[q], nearest[q] = v, k
    return link_fs, link_sf, nearest, best


def reference_over_q(fs, sf, sets):
    """reference(fs, sf, sets) with q as the array axis: an element-wise f32 `a + fs[:, y]` rounds once per element, so every chain
    is the scalar loop's; the members and the sets stay Python loops, in the same ascending order."""
    fs, sf = np.ascontiguousarray(fs, dtype=F), np.ascontiguousarray(sf, dtype=F)
    n1 = fs.shape[0]
    link_fs, link_sf = np.zeros((n1, len(sets)), F), np.zeros((n1, len(sets)), F)
    nearest, best = np.full(n1, NONE, np.uint32), np.full(n1, np.inf, F)
    with np.errstate(all="ignore"):
        for k, s in enumerate(sets):
            a, b = np.zeros(n1, F), np.zeros(n1, F)
            for y in sorted(s):
                a = a + fs[:, y]
                b = b + sf[y, :]
            link_fs[:, k] = a / F(F(1.0) * F(len(s)))
            link_sf[:, k] = b / F(F(len(s)) * F(1.0))
            for v in (link_fs[:, k], link_sf[:, k]):
                lower = v < best
                best[lower], nearest[lower] = v[lower], k
    assert link_fs.dtype == F and link_sf.dtype == F and best.dtype == F
    return link_fs, link_sf, nearest, best


def six_set_case():
    """(fs [37][333], sf [333][37], sets): six sets of 1 to 186 members, listed unsorted -- the case of
    tests/test_gpu_cross_linkage.py::test_linkage_matches_the_sequential_loop_bitwise."""
    rng = np.random.default_rng(20240607)
    n1, n2 = 37, 333
    fs = (rng.random((n1, n2), dtype=F) * F(9.0) + F(0.01)).astype(F)
    sf = (rng.random((n2, n1), dtype=F) * F(9.0) + F(0.01)).astype(F)
    perm = rng.permutation(n2)
    sizes, sets, at = (1, 2, 15, 64, 65, 186), [], 0
    for sz in sizes:
        sets.append([int(v) for v in perm[at:at + sz]])             # listed unsorted
        at += sz
    return fs, sf, sets


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    nan = np.isnan(want) if want.dtype == F else np.zeros(want.shape, bool)
    if want.dtype == F and not np.array_equal(np.isnan(got), nan):
        return False
    return np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def assert_equal(got, want, what):
    for g, w, name in zip(got, want, ("link_fs", "link_sf", "nearest", "nearest_linkage")):
        assert same_bits(g, w), "%s: %s differs from the sequential f32 loop" % (what, name)
