"""numpy-only reference of the cluster analysis (pbSimClusterStats / pbSimClusterLabelsOf, csrc/pb_cluster.hip).

Bots i != j are linked iff, in fp32 operation by operation,
    rx = xj - xi;  ry = yj - yi;  dist = sqrt(rx*rx + ry*ry);  (dist - (ri + rj)) < gap
A bot with a non-finite position or radius has no links.  A cluster is a connected component, a bot's label the smallest
original index of its component.  Candidate pairs come from this file's own cell binning (edge 1.01 (2 rmax + gap), the
half stencil of five cells), the components from min-label hooking plus pointer jumping.
tests/test_cluster_api.py pins all of it to an O(n^2) brute force."""
import numpy as np

f32 = np.float32
FIELDS = ("clusters", "largest", "largest_label", "isolated", "links", "max_degree")


def linked(xi, yi, ri, xj, yj, rj, gap):
    """The predicate on float32 arrays (or scalars), every operation rounded to fp32."""
    xi, yi, ri, xj, yj, rj = (np.asarray(a, f32) for a in (xi, yi, ri, xj, yj, rj))
    with np.errstate(all="ignore"):
        rx = xj - xi
        ry = yj - yi
        dist = np.sqrt(rx * rx + ry * ry)
        return (dist - (ri + rj)) < f32(gap)


def candidate_pairs(pos, rad, gap):
    """(i, j) index arrays, i != j, each unordered pair of finite bots closer than one cell at most once."""
    pos = np.asarray(pos, f32).reshape(-1, 2)
    rad = np.asarray(rad, f32)
    ok = np.isfinite(pos).all(axis=1) & np.isfinite(rad)
    idx = np.flatnonzero(ok)
    if idx.size < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    r = rad[idx].astype(np.float64)
    rmax = max(float(r.max()), 0.0)
    edge = max((2.0 * rmax + float(f32(gap))) * 1.01, 1e-3)
    p = pos[idx].astype(np.float64)
    cx = np.floor(p[:, 0] / edge).astype(np.int64)
    cy = np.floor(p[:, 1] / edge).astype(np.int64)
    kx = cx - cx.min() + 1
    ky = cy - cy.min()
    W = int(kx.max()) + 2
    key = ky * W + kx
    order = np.argsort(key, kind="stable")
    skey = key[order]
    sidx = idx[order]
    out_i, out_j = [], []
    m = skey.size
    for (dx, dy) in ((0, 0), (1, 0), (-1, 1), (0, 1), (1, 1)):
        want = skey + dy * W + dx
        lo = np.searchsorted(skey, want, side="left")
        hi = np.searchsorted(skey, want, side="right")
        if dx == 0 and dy == 0:
            lo = np.arange(m) + 1  # own cell: the bots behind this one
        cnt = np.maximum(hi - lo, 0)
        tot = int(cnt.sum())
        if tot == 0:
            continue
        a = np.repeat(np.arange(m), cnt)
        first = np.cumsum(cnt) - cnt
        b = np.arange(tot) - np.repeat(first, cnt) + np.repeat(lo, cnt)
        out_i.append(sidx[a])
        out_j.append(sidx[b])
    if not out_i:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(out_i), np.concatenate(out_j)


def links(pos, rad, gap):
    """The undirected links as (i, j) index arrays."""
    pos = np.asarray(pos, f32).reshape(-1, 2)
    rad = np.asarray(rad, f32)
    i, j = candidate_pairs(pos, rad, gap)
    keep = linked(pos[i, 0], pos[i, 1], rad[i], pos[j, 0], pos[j, 1], rad[j], gap)
    return i[keep], j[keep]


def components(n, i, j):
    """Labels (smallest index of the component) from min-label hooking plus pointer jumping."""
    lab = np.arange(n, dtype=np.int64)
    i = np.asarray(i, np.int64)
    j = np.asarray(j, np.int64)
    while i.size:
        li, lj = lab[i], lab[j]
        differ = li != lj
        i, j, li, lj = i[differ], j[differ], li[differ], lj[differ]
        if not i.size:
            break
        m = np.minimum(li, lj)
        np.minimum.at(lab, li, m)  # hook the roots
        np.minimum.at(lab, lj, m)
        while True:  # pointer jumping
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
    return lab


def stats_of(labels, degree):
    labels = np.asarray(labels, np.int64)
    degree = np.asarray(degree, np.int64)
    sizes = np.bincount(labels, minlength=labels.size)
    return {"clusters": int((sizes > 0).sum()), "largest": int(sizes.max()),
            "largest_label": int(np.argmax(sizes)),  # the first maximum: the smallest label among ties
            "isolated": int((degree == 0).sum()), "links": int(degree.sum() // 2), "max_degree": int(degree.max())}


def analyse(pos, rad, gap):
    """(stats dict, labels uint32, degree uint32) of one member's state."""
    rad = np.asarray(rad, f32)
    n = rad.size
    i, j = links(pos, rad, gap)
    degree = np.bincount(i, minlength=n) + np.bincount(j, minlength=n)
    labels = components(n, i, j)
    try:  # a cross-check when scipy is there; never needed
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        k, comp = connected_components(coo_matrix((np.ones(i.size, np.int8), (i, j)), shape=(n, n)), directed=False)
        assert k == np.unique(labels).size and np.unique(np.stack([comp, labels]), axis=1).shape[1] == k
    except ImportError:
        pass
    return stats_of(labels, degree), labels.astype(np.uint32), degree.astype(np.uint32)


def nontrivial(stats, n):
    return 1 < stats["clusters"] < n and stats["largest"] > 1
