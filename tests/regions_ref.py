"""CPU restatement (numpy) of the per-sphere regions of the weak-label sampler, the yardstick of tests/test_regions_*.py and
the fixture source of tools/region_loss_ab.py.  Written from datasets/DALES_WeakLabel.py:424-451 and :474-476 on ASCENDING
`input_inds` (the sampler's order), with the contract of include/weasal_hip.h: the candidates of a sphere are the anchors with
d2 = (dx*dx + dy*dy) + dz*dz <= r*r in float64 (numpy rounds every product and sum), r = in_radius - sub_radius - 0.01; a region
is the positions, in the sphere's slice, of the anchor's members that occur there (np.isin + np.searchsorted); it is dropped
unless `idx.any()`; kept regions are in ascending anchor order.  Distances are brute force; nothing here touches the device
library or sklearn.  Plus the two formulas of the region means in float64.  This file holds no tests.

An anchor set is (lists, lb, centres): ascending int64 index arrays, 0/1 label rows [A, C], float64 centres [A, 3].
"""
import numpy as np


def search_radius(in_radius, sub_radius):
    """:434, in float64 as written"""
    return float(in_radius) - float(sub_radius) - 0.01


def candidates(anchor_centres, centre, r):
    """ascending anchor ids with d2 <= r*r"""
    c = np.asarray(anchor_centres, np.float64).reshape(-1, 3)
    d = c - np.asarray(centre, np.float64).reshape(1, 3)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return np.nonzero(d2 <= np.float64(r) * np.float64(r))[0]


def region_of(members, input_inds):
    """:445-448 on ascending input_inds: the sphere-local rows of the members inside the sphere, or None when dropped (:449)"""
    members = np.asarray(members, np.int64)
    input_inds = np.asarray(input_inds, np.int64)
    y = members[np.isin(members, input_inds)]
    idx = np.searchsorted(input_inds, y)
    return idx.astype(np.int64) if idx.any() else None


def sphere_regions(anchor_set, centre, input_inds, r):
    """-> (anchor ids, local index arrays, label rows) of the kept regions of one sphere, ascending anchor id"""
    lists, lb, centres = anchor_set
    ids, regions, rows = [], [], []
    for a in candidates(centres, centre, r):
        idx = region_of(lists[a], input_inds)
        if idx is not None:
            ids.append(int(a))
            regions.append(idx)
            rows.append(np.asarray(lb[a], np.float32))
    return ids, regions, rows


def cut(anchor_sets, cloud_inds, centres, input_inds, lengths, labels, in_radius, sub_radius, n_class):
    """the whole batch -> dict(ptr, idx, sphere, anchor, lb, inv_len, cloud_lb, region, region_lb): the CSR of
    regions.SphereRegions (idx = rows of the stacked batch) and the reference's per-sphere lists"""
    lengths = np.asarray(lengths, np.int64)
    input_inds = np.asarray(input_inds, np.int64)
    labels = np.asarray(labels, np.int64)
    if len(labels) and (labels.min() < 0 or labels.max() >= n_class):
        raise ValueError("label outside [0, n_class)")
    r = search_radius(in_radius, sub_radius)
    row_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ptr, idx, sphere, anchor, lb, region, region_lb = [0], [], [], [], [], [], []
    cloud_lb = np.zeros((len(lengths), n_class), np.float32)
    for s in range(len(lengths)):
        sl = slice(row_off[s], row_off[s + 1])
        cloud_lb[s, np.unique(labels[sl])] = 1                                   # :474-476
        ids, regs, rows = sphere_regions(anchor_sets[int(cloud_inds[s])], centres[s], input_inds[sl], r) if r >= 0 else ([], [], [])
        region.append(regs)
        region_lb.append(rows)
        for a, g, row in zip(ids, regs, rows):
            idx.append(g + row_off[s])
            ptr.append(ptr[-1] + len(g))
            sphere.append(s)
            anchor.append(a)
            lb.append(row)
    ptr = np.asarray(ptr, np.int64)
    lens = np.diff(ptr)
    return dict(ptr=ptr, idx=np.concatenate(idx + [np.zeros(0, np.int64)]).astype(np.int64), sphere=np.asarray(sphere, np.int32),
                anchor=np.asarray(anchor, np.int64), lb=np.asarray(lb, np.float32).reshape(-1, n_class),
                inv_len=(np.float32(1.0) / lens.astype(np.float32)).astype(np.float32), cloud_lb=cloud_lb, region=region,
                region_lb=region_lb)


def transpose(ptr, idx, n):
    """point -> regions: (t_ptr int64 [n + 1], t_reg int32 [nnz] ascending per point)"""
    ptr, idx = np.asarray(ptr, np.int64), np.asarray(idx, np.int64)
    reg = np.repeat(np.arange(len(ptr) - 1, dtype=np.int32), np.diff(ptr))
    order = np.argsort(idx, kind='stable')
    t_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(idx, minlength=n), out=t_ptr[1:])
    return t_ptr, reg[order]


def region_mean64(x, ptr, idx):
    """(mean [R, W], mean of |x| [R, W]) in float64: out[r] = sum of x[idx[i]] over the region / its length"""
    x = np.asarray(x, np.float64)
    out = np.zeros((len(ptr) - 1, x.shape[1]), np.float64)
    mag = np.zeros_like(out)
    for r in range(len(ptr) - 1):
        rows = x[idx[ptr[r]:ptr[r + 1]]]
        out[r] = rows.sum(axis=0) / rows.shape[0]
        mag[r] = np.abs(rows).sum(axis=0) / rows.shape[0]
    return out, mag


def region_mean_grad64(g, ptr, idx, inv_len, n):
    """(dx [n, W], sum of |g_r| * inv_len_r [n, W], regions per row [n]) in float64; inv_len [R]: the weights, e.g. the exact
    1 / length"""
    g = np.asarray(g, np.float64)
    w = np.asarray(inv_len, np.float64)
    dx = np.zeros((n, g.shape[1]), np.float64)
    mag = np.zeros_like(dx)
    m = np.zeros(n, np.int64)
    for r in range(len(ptr) - 1):
        rows = idx[ptr[r]:ptr[r + 1]]
        dx[rows] += g[r] * w[r]
        mag[rows] += np.abs(g[r]) * w[r]
        m[rows] += 1
    return dx, mag, m


# ------------------------------------------------------------------------------------------------------------------
# fixtures shared by the tests and tools/region_loss_ab.py
# ------------------------------------------------------------------------------------------------------------------
def pack_bits(lb):
    lb = np.asarray(lb, np.uint64)
    return (lb << np.arange(lb.shape[1], dtype=np.uint64)).sum(axis=1, dtype=np.uint64).astype(np.uint32)


def csr(lists):
    ptr = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(l) for l in lists], out=ptr[1:])
    return ptr, np.concatenate([np.asarray(l, np.int64) for l in lists] + [np.zeros(0, np.int64)])


def sphere_inds(points, centre, in_radius):
    """ascending ids of the float32 points (widened) within in_radius of the float64 centre: the sampler's members"""
    d = np.asarray(points, np.float32).astype(np.float64) - np.asarray(centre, np.float64)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return np.nonzero(d2 <= np.float64(in_radius) * np.float64(in_radius))[0].astype(np.int64)


IN_RADIUS, SUB_RADIUS, N_CLASS = 10.0, 4.0, 9


def edge_batch(seed=17):
    """A hand-built batch of five spheres over three tiles, with anchor sets made directly from arrays so that every case
    exists by construction (the member lists are free: nothing here needs them to be balls).  -> dict with
      tiles [(points float32 [M, 3], labels int64 [M])], anchor_sets [(lists, lb, centres)], cloud_inds, centres (float64),
      input_inds / labels (the stacked batch), lengths, in_radius, sub_radius, n_class, cases (anchor ids by name).
    Spheres, in batch order: 0 tile 0 at the origin; 1 tile 1; 2 tile 0 far away, no candidate anchor; 3 tile 2, whose anchor
    set is empty; 4 tile 0 again, one unit along x.  Tile 0 (1 461 points): point 0 lies next to the origin, so it is local
    row 0 of spheres 0 and 4.  Its anchors: `row0_only` {0}; `row0_more` {0 and others}; `single` one member that is not row
    0; `n64`, `n65`, `n257`, `n1100` that many members inside sphere 0; `outside` members all beyond the sphere; `partly` half
    in, half out; `on_radius` a centre exactly at the search radius of sphere 0 and `ulp_out` one float64 ulp beyond;
    `repeat` the same anchor as `n64` again; `far` a candidate of no sphere."""
    rng = np.random.RandomState(seed)

    def ball(n, radius, centre, inner=0.0):
        v = rng.normal(size=(n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        rad = (inner ** 3 + rng.uniform(0, 1, size=(n, 1)) * (radius ** 3 - inner ** 3)) ** (1 / 3)
        return (v * rad + np.asarray(centre, np.float64)).astype(np.float32)

    r = search_radius(IN_RADIUS, SUB_RADIUS)
    # ---- tile 0
    body = np.concatenate([ball(1300, 9.5, (0, 0, 0)), ball(60, 5.0, (100, 0, 0)), ball(100, 15.0, (0, 0, 0), inner=12.0)])
    body = body[rng.permutation(body.shape[0])]
    p0 = np.concatenate([np.array([[0.5, 0, 0]], np.float32), body])
    l0 = rng.randint(0, N_CLASS, size=p0.shape[0]).astype(np.int64)
    c_a, c_b, c_far = np.zeros(3), np.array([1.0, 0, 0]), np.array([100.0, 0, 0])
    in_a = sphere_inds(p0, c_a, IN_RADIUS)
    assert in_a[0] == 0 and sphere_inds(p0, c_b, IN_RADIUS)[0] == 0
    rest = in_a[1:]
    out_a = np.setdiff1d(np.arange(p0.shape[0]), np.union1d(in_a, sphere_inds(p0, c_b, IN_RADIUS)))
    out_a = out_a[np.linalg.norm(p0[out_a].astype(np.float64), axis=1) < 50]             # the shell, not the far cluster
    names, lists, cen = [], [], []

    def pick(k):
        return np.sort(rng.choice(rest, size=k, replace=False)).astype(np.int64)

    def add(name, members, centre):
        names.append(name)
        lists.append(np.asarray(members, np.int64))
        cen.append(np.asarray(centre, np.float64))

    add('row0_only', [0], (0, 0, 0))
    add('row0_more', np.concatenate([[0], pick(5)]), (1, 0, 0))
    add('single', pick(1), (0, 1, 0))
    add('n64', pick(64), (0, 0, 1))
    add('n65', pick(65), (0, 0, -1))
    add('n257', pick(257), (0, -1, 0))
    add('n1100', pick(1100), (-1, 0, 0))
    add('outside', out_a[:30], (2, 0, 0))
    add('partly', np.sort(np.concatenate([pick(20), out_a[30:50]])), (0, 2, 0))
    add('on_radius', pick(7), (r, 0, 0))
    add('ulp_out', pick(9), (np.nextafter(r, np.inf), 0, 0))
    add('repeat', lists[names.index('n64')], (0, 0, 1))
    add('far', pick(3), (300, 0, 0))
    assert r * r < np.nextafter(r, np.inf) * np.nextafter(r, np.inf)                      # the ulp shows in the rounded squares
    lb0 = rng.randint(0, 2, size=(len(lists), N_CLASS)).astype(np.int64)
    # ---- tile 1 (small) and tile 2 (its anchor set is empty)
    p1 = ball(70, 3.0, (0, 0, 0))
    l1 = rng.choice([2, 5], size=70).astype(np.int64)
    lists1 = [np.arange(1, 21, dtype=np.int64), np.array([0], np.int64), np.arange(30, 40, dtype=np.int64)]
    cen1 = np.array([[0, 0, 0], [0, 0, 2], [50, 0, 0]], np.float64)
    lb1 = rng.randint(0, 2, size=(3, N_CLASS)).astype(np.int64)
    p2 = ball(40, 3.0, (0, 0, 0))
    l2 = rng.randint(0, N_CLASS, size=40).astype(np.int64)
    tiles = [(p0, l0), (p1, l1), (p2, l2)]
    anchor_sets = [(lists, lb0, np.asarray(cen, np.float64)), (lists1, lb1, cen1),
                   ([], np.zeros((0, N_CLASS), np.int64), np.zeros((0, 3), np.float64))]
    cloud_inds = np.array([0, 1, 0, 2, 0], np.int64)
    centres = np.array([c_a, [0, 0, 0], c_far, [0, 0, 0], c_b], np.float64)
    inds = [sphere_inds(tiles[t][0], c, IN_RADIUS) for t, c in zip(cloud_inds, centres)]
    lengths = np.array([len(i) for i in inds], np.int64)
    labels = np.concatenate([tiles[t][1][i] for t, i in zip(cloud_inds, inds)])
    return dict(tiles=tiles, anchor_sets=anchor_sets, cloud_inds=cloud_inds, centres=centres, input_inds=np.concatenate(inds),
                labels=labels, lengths=lengths, in_radius=IN_RADIUS, sub_radius=SUB_RADIUS, n_class=N_CLASS,
                cases={n: i for i, n in enumerate(names)})
