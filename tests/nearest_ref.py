"""tests/nearest_ref.py -- the reference of the exact nearest-neighbour search (ws_nearest_neighbors).

What sklearn's KDTree.query(points, k=1) computes (datasets/DALES_PseudoLabel.py:888-893), as a chunked float64 brute force
in numpy: per batch element, for every query the support that minimises (d2, index) with
    d2 = ((dx*dx) + (dy*dy)) + (dz*dz),   dx = float64(q.x) - float64(s.x)
(numpy rounds every product and sum: no FMA), np.lexsort on (index, d2) deciding.  A support with a non-finite d2 is never
chosen; a query with a non-finite coordinate, and every query of an element without supports, gets ns and +inf.
"""
import numpy as np


def nearest_ref(queries, supports, q_lens, s_lens, chunk=512):
    """-> (index int64 [nq] (global, ns = none), d2 float64 [nq] (+inf = none))"""
    q64 = np.asarray(queries, np.float32).reshape(-1, 3).astype(np.float64)
    s64 = np.asarray(supports, np.float32).reshape(-1, 3).astype(np.float64)
    nq, ns = q64.shape[0], s64.shape[0]
    assert int(np.sum(q_lens)) == nq and int(np.sum(s_lens)) == ns and len(q_lens) == len(s_lens)
    idx = np.full(nq, ns, np.int64)
    best = np.full(nq, np.inf, np.float64)
    q0 = s0 = 0
    for ql, sl in zip(q_lens, s_lens):
        ql, sl = int(ql), int(sl)
        S = s64[s0:s0 + sl]
        gidx = np.arange(s0, s0 + sl, dtype=np.int64)
        for a in range(q0, q0 + ql if sl else q0, chunk):
            Q = q64[a:min(a + chunk, q0 + ql)]
            with np.errstate(invalid="ignore", over="ignore"):
                dx = Q[:, None, 0] - S[None, :, 0]
                dy = Q[:, None, 1] - S[None, :, 1]
                dz = Q[:, None, 2] - S[None, :, 2]
                d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
            d2 = np.where(np.isfinite(d2), d2, np.inf)
            for r in range(Q.shape[0]):
                j = np.lexsort((gidx, d2[r]))[0]
                if d2[r, j] < np.inf and np.all(np.isfinite(Q[r])):
                    idx[a + r], best[a + r] = gidx[j], d2[r, j]
        q0 += ql
        s0 += sl
    return idx, best
