#!/usr/bin/env python3
"""tests/golden/make_golden_nearest.py -- fixture of the exact nearest-neighbour search: what
sklearn.neighbors.KDTree(leaf_size=10).query returns (the reference's call, datasets/DALES_PseudoLabel.py:888-893) for the
points of two small clouds against their grid barycentres.  Output (data, not source): g22_nearest.npz
  queries  f32 [5000, 3]   3000 + 2000 points, offset like a real tile's coordinates (3000, 5000, 100), on a 1/256 m raster
                           (as laser returns are; it also keeps the file small)
  supports f32 [1215, 3]   the barycentres of their dl = 0.5 cells, cloud by cloud
  q_lens, s_lens           the batch
  idx      int32 [5000]    the tree's nearest support (GLOBAL index into supports), per cloud
  dist     f64 [5000]      its distance
  tie_free bool [5000]     dist[:, 0] < dist[:, 1] of query(k=2): rows where the tree's answer is not implementation-defined
Asserted here: the mask excludes at most 0.1 % of the rows.  Needs numpy and sklearn only."""
import os

import numpy as np
from sklearn.neighbors import KDTree

HERE = os.path.dirname(os.path.abspath(__file__))


def barycentres(points, dl):
    key = np.floor(points / np.float32(dl)).astype(np.int64)
    _, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    m = int(inv.max()) + 1
    cnt = np.bincount(inv, minlength=m)
    sub = np.stack([np.bincount(inv, weights=points[:, c].astype(np.float64), minlength=m) for c in range(3)], axis=1)
    return (sub / cnt[:, None]).astype(np.float32)


def main():
    rng = np.random.default_rng(22)
    dl, off = 0.5, np.array([3000.0, 5000.0, 100.0])
    queries, supports, idx, dist, free, q_lens, s_lens = [], [], [], [], [], [], []
    base = 0
    for n, box in ((3000, (5.5, 5.5, 3.0)), (2000, (5.0, 5.0, 2.5))):
        p = (np.round(rng.uniform(0, 1, (n, 3)) * np.array(box) * 256) / 256 + off).astype(np.float32)
        s = barycentres(p, dl)
        d, i = KDTree(s, leaf_size=10).query(p, k=2, return_distance=True)
        queries.append(p); supports.append(s); q_lens.append(n); s_lens.append(s.shape[0])
        idx.append(i[:, 0] + base); dist.append(d[:, 0]); free.append(d[:, 0] < d[:, 1])
        base += s.shape[0]
    free = np.concatenate(free)
    assert (~free).sum() <= 1e-3 * free.shape[0], int((~free).sum())
    out = os.path.join(HERE, "g22_nearest.npz")
    np.savez_compressed(out, queries=np.concatenate(queries), supports=np.concatenate(supports),
                        q_lens=np.array(q_lens, np.int32), s_lens=np.array(s_lens, np.int32),
                        idx=np.concatenate(idx).astype(np.int32), dist=np.concatenate(dist), tie_free=free, dl=np.float32(dl))
    print("supports", s_lens, "ties", int((~free).sum()), "bytes", os.path.getsize(out))
    assert os.path.getsize(out) < 100_000


if __name__ == "__main__":
    main()
