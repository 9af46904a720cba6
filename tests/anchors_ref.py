"""CPU restatement (numpy) of the weak-label anchors, the yardstick of tests/test_anchors_*.py and the fixture source of
tools/anchors_bench.py.  Written from the arithmetic of utils/anchors.py:26-73 (lattice), :75-103 (members and label rows),
:105-143 (overlap anchors) and :145-268 (selection), with the contract of include/weasal_hip.h: a float32 coordinate widened
to float64, d2 = (dx*dx + dy*dy) + dz*dz (numpy rounds every product and sum), inside iff d2 <= radius*radius.  Distances
are brute force; nothing here touches the device library or sklearn.

Anchors are Python lists of ascending int64 index arrays with 0/1 label rows [A, C]; overlap anchors follow the inputs in
(i, j) lexicographic order of their pair.
"""
import random

import numpy as np


def d2_to(points, centre):
    """float64 [N]: squared distances of float32 points (widened) to one float64 centre, the contract's recipe"""
    d = np.asarray(points, np.float32).astype(np.float64) - np.asarray(centre, np.float64)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def get_anchors(points, sub_radius, method='full'):
    """float64 [A0, 3] (:26-73): float32 extents widened to float64 for the counts, np.linspace in float64, nested x, y, z"""
    p = np.asarray(points, np.float32)
    if method not in ('full', 'reduced'):
        raise ValueError('Unsupported method (' + method + ') for creating anchor points')
    spacing = float(sub_radius) if method == 'full' else float(2 * sub_radius)
    axes = []
    for d in range(3):
        lo, hi = p[:, d].min(), p[:, d].max()
        extent = float(np.float32(hi - lo))
        axes.append(np.linspace(float(lo), float(hi), int(np.floor(extent / spacing) + 1)))
    out = []
    for x in axes[0]:
        for y in axes[1]:
            for z in axes[2]:
                out.append([x, y, z])
                if method == 'reduced':
                    out.append([x, y, z + sub_radius])
                    out.append([x + sub_radius, y + sub_radius, z])
                    out.append([x + sub_radius, y + sub_radius, z + sub_radius])
    return np.array(out, np.float64).reshape(-1, 3)


def anchors_with_points(points, labels, anchors, radius, n_class):
    """-> (kept int64 [A], lists, centres float64 [A, 3], lb int64 [A, n_class]) (:75-103)"""
    anchors = np.asarray(anchors, np.float64).reshape(-1, 3)
    labels = np.asarray(labels)
    if len(labels) and (labels.min() < 0 or labels.max() >= n_class):
        raise ValueError("label outside [0, n_class)")
    r2 = np.float64(radius) * np.float64(radius)
    kept, lists, rows = [], [], []
    for a in range(anchors.shape[0]):
        members = np.nonzero(d2_to(points, anchors[a]) <= r2)[0].astype(np.int64)
        if members.shape[0] > 0:
            kept.append(a)
            lists.append(members)
            row = np.zeros(n_class, np.int64)
            row[np.unique(labels[members])] = 1
            rows.append(row)
    kept = np.asarray(kept, np.int64)
    return kept, lists, anchors[kept], np.asarray(rows, np.int64).reshape(-1, n_class)


def candidate_pairs(centres, sub_radius):
    """[(i, j)] with i < j and the centres within 1.5 * sub_radius, lexicographic (:114-121)"""
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    reach = np.float64(1.5 * float(sub_radius))
    r2 = reach * reach
    pairs = []
    for i in range(c.shape[0]):
        d = c[i + 1:] - c[i]                                   # (the sign of a difference does not change its square)
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        pairs += [(i, i + 1 + int(k)) for k in np.nonzero(d2 <= r2)[0]]
    return pairs


def update_anchors(points, lists, centres, lb, sub_radius, use_anchors=None):
    """-> (lists, centres, lb, n_base) of the selected anchors followed by the overlap anchors (:105-143 after :145-160)"""
    p64 = np.asarray(points, np.float32).astype(np.float64)
    lb = np.asarray(lb, np.int64)
    centres = np.asarray(centres, np.float64).reshape(-1, 3)
    if use_anchors is not None:
        sel = np.asarray(use_anchors, np.int64)
        if len(sel) and (sel.min() < 0 or sel.max() >= len(lists)):
            raise ValueError("use_anchors outside [0, A)")
        lists, centres, lb = [lists[a] for a in sel], centres[sel], lb[sel]
    n_base = len(lists)
    out_lists, out_centres, out_lb = list(lists), [c for c in centres], [r for r in lb]
    for i, j in candidate_pairs(centres, sub_radius):
        if (lb[i] != lb[j]).sum() == 0:
            continue
        common = np.intersect1d(lists[i], lists[j])
        if common.shape[0] < 1:
            continue
        out_lists.append(common.astype(np.int64))
        out_centres.append(np.mean(p64[common], axis=0))
        out_lb.append(lb[i] * lb[j])
    return out_lists, np.asarray(out_centres, np.float64).reshape(-1, 3), np.asarray(out_lb, np.int64).reshape(-1, lb.shape[1]), n_base


def pack_bits(lb):
    lb = np.asarray(lb, np.uint64)
    return (lb << np.arange(lb.shape[1], dtype=np.uint64)).sum(axis=1, dtype=np.uint64).astype(np.uint32)


def subsample_indices(lb, anchor_count, method):
    """`anchor_inds_sub` of :162-262 for label rows [A, C]; draws from Python's `random`"""
    lb = np.asarray(lb)
    total = len(lb)
    if anchor_count > total:
        raise ValueError('Selected anchor count (' + str(anchor_count) + ') exceeds the number of anchors (' + str(total) + ')!')
    if method == 'regular':
        return list(np.round(np.linspace(0, total - 1, anchor_count)).astype(int))
    if method == 'random':
        return sorted(random.choices(list(range(total)), k=anchor_count))
    if method != 'balanced':
        raise ValueError('Subsample method "' + method + '" is not supported!')
    left = list(range(total))
    out = []
    todo = anchor_count
    for _ in range(4):
        per_class = {k: [a for a in left if lb[a][k] == 1] for k in range(lb.shape[1])}
        each = int(todo / len(per_class))
        add = []
        for k in per_class:
            if len(per_class[k]) >= each:
                add += [per_class[k][i] for i in np.round(np.linspace(0, len(per_class[k]) - 1, each)).astype(int)]
            else:
                add += per_class[k]
        add = set(add)
        out += list(add)
        left = [a for a in left if a not in add]
        todo = anchor_count - len(out)
        if todo < len(per_class):
            break
    out += random.choices(left, k=todo)
    return sorted(out)


# ------------------------------------------------------------------------------------------------------------------
# fixtures shared by the tests and tools/anchors_bench.py
# ------------------------------------------------------------------------------------------------------------------
RADIUS = 5.0


def edge_cloud(n_class=9, seed=7):
    """(points float32 [N, 3], labels int32 [N], anchors float64 [A0, 3]) around radius 5 with, by construction:
    empty anchors first and last and in between; an anchor with more than 1024 members and a neighbour that shares them
    under another label row; one with more than 256; one with exactly one; a point exactly on a boundary ((3, 4, 0) from
    (0, 0, 0)) and one a float64 ulp outside; neighbouring pairs with equal rows, with differing rows and no common point,
    with differing rows and one common point; a random slab under a 'reduced' lattice.  N is no multiple of 64."""
    rng = np.random.RandomState(seed)
    pts, lab, anc = [], [], []

    def add(p, l):
        p = np.asarray(p, np.float32).reshape(-1, 3)
        pts.append(p)
        lab.append(np.broadcast_to(np.asarray(l, np.int32), (p.shape[0],)).copy())

    anc.append([1000.0, 1000.0, 1000.0])                                        # 0: empty, first
    anc.append([0.0, 0.0, 0.0])                                                 # 1: (3, 4, 0) is exactly on its boundary
    add([[3, 4, 0], [0, 0, 1]], [2, 2])
    add(np.array([50, 0, 0]) + rng.uniform(-0.55, 0.55, size=(1100, 3)), 0)     # > 1024 members
    anc.append([50.0, 0.0, 0.0])                                                # 2
    anc.append([53.0, 0.0, 0.0])                                                # 3: shares the cluster, other row
    add([[57, 0, 0]], 1)
    anc.append([-500.0, 0.0, 0.0])                                              # 4: empty, in between
    add(np.array([100, 0, 0]) + rng.uniform(-0.55, 0.55, size=(300, 3)), rng.randint(0, 3, size=300))
    anc.append([100.0, 0.0, 0.0])                                               # 5: > 256 members
    anc.append([200.0, 0.0, 0.0])                                               # 6: exactly one member
    add([[200, 1, 0]], 3)
    anc.append([400.0, -2.0 ** -50, 0.0])                                       # 7: (400, 5, 0) is one ulp of 5 outside
    add([[400, 5, 0], [400, 0, 0]], [4, 5])
    anc.append([300.0, 0.0, 0.0])                                               # 8, 9: equal rows, common points
    anc.append([302.0, 0.0, 0.0])
    add([[301, 0, 0], [301, 1, 0]], [6, 7])
    anc.append([500.0, 0.0, 0.0])                                               # 10, 11: differing rows, nothing in common
    anc.append([507.0, 0.0, 0.0])
    add([[497, 0, 0], [510, 0, 0]], [0, 1])
    anc.append([600.0, 0.0, 0.0])                                               # 12, 13: differing rows, one common point
    anc.append([607.0, 0.0, 0.0])
    add([[603.5, 0, 0], [596, 0, 0]], [0, 1])
    slab = (np.array([700, 0, 0]) + rng.uniform(0, 1, size=(1590, 3)) * np.array([50, 40, 8])).astype(np.float32)
    add(slab, rng.randint(0, n_class, size=slab.shape[0]))
    lattice = get_anchors(slab, RADIUS, 'reduced')
    anchors = np.concatenate([np.asarray(anc, np.float64), lattice, [[-1000.0, -1000.0, -1000.0]]])     # empty, last
    points = np.concatenate(pts).astype(np.float32)
    labels = np.concatenate(lab).astype(np.int32)
    order = rng.permutation(points.shape[0])                                   # members of an anchor are not contiguous
    assert points.shape[0] % 64 != 0
    return points[order], labels[order], anchors


def golden_cloud(seed=16, n=2400):
    """(points float32 [n, 3], labels int32 [n]) of the golden g16_anchors.npz: a 42 m x 36 m x 9 m slab, nine classes"""
    rng = np.random.RandomState(seed)
    points = (rng.uniform(0, 1, size=(n, 3)) * np.array([42.0, 36.0, 9.0]) + np.array([10.0, -5.0, 2.0])).astype(np.float32)
    labels = (np.floor(points[:, 0] / 7.0) + rng.randint(0, 2, size=n)).astype(np.int32) % 9
    return points, labels
