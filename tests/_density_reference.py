"""The contract of apd_density_clusters (include/apd.h) restated in numpy: test infrastructure, shares no code with the library.

    density_reference(d, eps, min_pts, link)  ->  labels, kind, degree, counts, nans   for ONE setting

The comparison is made in float32 (numpy's `<=` on float32 arrays is the IEEE one: NaN never, -0.0 == +0.0, +INF <= +INF), the
adjacency is an [n][n] boolean matrix, the components come from a stack search started at every unlabelled core point in ascending
number -- so the start is the smallest core point of its component -- and the border rule, the counts and the NaN count follow the
header's text.  Also the generators the density tests share."""
import numpy as np

F = np.float32
EITHER, BOTH = 0, 1
NOISE, BORDER, CORE = 0, 1, 2


def adjacency(d, eps, link):
    d = np.asarray(d, F)
    n = d.shape[0]
    with np.errstate(invalid="ignore"):
        near = d <= F(eps)
    adj = (near | near.T) if link == EITHER else (near & near.T)
    adj[np.arange(n), np.arange(n)] = False                                   # the diagonal's value enters nothing
    return adj


def density_reference(d, eps, min_pts, link=EITHER):
    d = np.asarray(d, F)
    n = d.shape[0]
    assert d.shape == (n, n) and int(min_pts) >= 1 and link in (EITHER, BOTH)
    adj = adjacency(d, eps, link)
    degree = adj.sum(axis=1).astype(np.uint32)
    core = degree.astype(np.uint64) + 1 >= np.uint64(min_pts)
    labels = np.arange(n, dtype=np.uint32)
    seen = np.zeros(n, bool)
    for start in range(n):                                                    # ascending: `start` is the smallest of its component
        if not core[start] or seen[start]:
            continue
        stack = [start]
        seen[start] = True
        while stack:
            i = stack.pop()
            labels[i] = start
            for j in np.flatnonzero(adj[i] & core & ~seen):
                seen[j] = True
                stack.append(int(j))
    kind = np.where(core, CORE, NOISE).astype(np.uint8)
    for i in np.flatnonzero(~core):
        mine = np.flatnonzero(adj[i] & core)
        if len(mine):
            kind[i] = BORDER
            labels[i] = labels[mine].min()
    clusters = len(np.unique(labels[core]))
    counts = np.array([clusters, (kind == CORE).sum(), (kind == BORDER).sum(), (kind == NOISE).sum()], np.uint32)
    off = ~np.eye(n, dtype=bool)
    nans = int(np.isnan(d[off]).sum()) if n else 0
    return labels, kind, degree, counts, nans


def density_sets_reference(labels, kind):
    """(members, set_off) by the definition: noise left out, the sets ascending by label, the members ascending."""
    labels, kind = np.asarray(labels), np.asarray(kind)
    members, set_off = [], [0]
    for lab in sorted(set(int(v) for v, k in zip(labels, kind) if k != NOISE)):
        members += [i for i in range(len(labels)) if kind[i] != NOISE and labels[i] == lab]
        set_off.append(len(members))
    return np.array(members, np.uint32), np.array(set_off, np.uint32)


def blob_points(n, seed, background=0.2, spread=0.25):
    """Seeded 2-D blobs around four jittered centres of a 5 x 5 square, plus a fifth of uniform background, in random order."""
    rng = np.random.default_rng(seed)
    n_bg = int(round(n * background))
    mids = np.array([[1, 1], [1, 4], [4, 1], [4, 4]], float) + rng.uniform(-0.3, 0.3, (4, 2))
    pts = mids[rng.integers(0, 4, n - n_bg)] + rng.standard_normal((n - n_bg, 2)) * spread
    pts = np.concatenate([pts, rng.uniform(0.0, 5.0, (n_bg, 2))])
    return pts[rng.permutation(n)]


def blob_matrix(n, seed, asymmetric=False):
    """Euclidean distances of blob_points in float32; asymmetric: the two triangles perturbed independently (up to +-15 %)."""
    if n == 0:
        return np.zeros((0, 0), F)
    pts = blob_points(n, seed)
    d = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    if asymmetric:
        d = d * np.random.default_rng(seed + 1000).uniform(0.85, 1.15, (n, n))
    d = d.astype(F)
    np.fill_diagonal(d, 0.0)
    return np.ascontiguousarray(d)


def border_tie_matrix():
    """Points 1, 2, 3 and 4, 5, 6 are two triangles at distance 0.5; point 0 is near 6 and 2 only.  With min_pts = 4 the cores are 2
    and 6 (three neighbours each), and 0 is a border point that sees both clusters."""
    d = np.full((7, 7), 9.0, F)
    for group in ((1, 2, 3), (4, 5, 6)):
        for i in group:
            for j in group:
                d[i, j] = 0.5
    d[0, 6] = d[6, 0] = d[0, 2] = d[2, 0] = 0.5
    np.fill_diagonal(d, 0.0)
    return d


def chain_matrix(order, n, near=F(0.25), far=F(9.0)):
    """A path graph over the points `order` among n: d[order[t]][order[t + 1]] is small (one direction only), everything else large."""
    order = np.asarray(order)
    d = np.full((n, n), far, F)
    d[order[:-1], order[1:]] = near
    np.fill_diagonal(d, 0.0)
    return d
