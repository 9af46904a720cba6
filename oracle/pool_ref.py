"""oracle/pool_ref.py -- TEST INFRASTRUCTURE ONLY (numpy).

References of the pooling kernels (weasal_amd/csrc/pools.hip) and of the transposed table every backward gathers through
(csr.hip, scan.hip), for tests/test_pool_branches_*.py.  Written from the kernels' contracts (include/weasal_hip.h) and the
meaning of models/blocks.py:80-111:

  max_pool      out[q, ch] = max over the h columns of x_pad[inds[q, col], ch], x_pad = x with a zero row appended (the
                shadow row: every index outside [0, ns) reads it).  arg[q, ch] = the FIRST column that attains the
                maximum; the backward routes dy[q, ch] to the support of that column alone (nothing when that column is
                a shadow column).
  closest_pool  out[q] = x_pad[inds[q, 0]]; the backward sums dy[q] into support inds[q, 0].
  table         offsets [ns + 2], pairs: the flat pair ids q * h + col of support s are pairs[offsets[s] : offsets[s + 1]],
                ascending.  Shadow pairs are not tabulated: slot ns stays empty, offsets[ns + 1] == offsets[ns] == the
                number of real pairs (include/weasal_hip.h, ws_transpose_build).

Error model of the backward sums (u = 2^-24): the kernels add the n contributing terms of an element in f32, in some order
(a sequential chain; the vector closest-pool form adds S partial chains through a log2(S)-deep tree, at most 6 levels; one more
addition for `add`): |got - ref| <= (n + 8) u sum|terms|.  A bf16 store rounds the f32 result once:
bound * (1 + 2^-8) + 2^-8 |ref| (the model of oracle/gemm_branch_ref.py).  Never a fraction of the tensor's maximum.
"""
import numpy as np

U = 2.0 ** -24
C_TREE = 8.0


def _live(inds, ns):
    inds = np.asarray(inds)
    return (inds >= 0) & (inds < ns)


def _padded(x):
    x = np.asarray(x)
    return np.concatenate([x, np.zeros((1, x.shape[1]), x.dtype)], 0)


# ------------------------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------------------------
def max_pool_ref(x, inds):
    """(out [nq, c] in x's dtype, arg [nq, c] int32): arg = the first column that attains the maximum"""
    x = np.asarray(x)
    inds = np.asarray(inds)
    ns = x.shape[0]
    idx = np.where(_live(inds, ns), inds, ns)
    vals = _padded(x)[idx]                                   # [nq, h, c]
    out = vals.max(1)
    first = (vals == out[:, None, :]).argmax(1)              # first True along the columns: stated, no library tie rule
    return out, first.astype(np.int32)


def closest_pool_ref(x, inds):
    x = np.asarray(x)
    inds = np.asarray(inds)
    ns = x.shape[0]
    col0 = inds[:, 0]
    return _padded(x)[np.where(_live(col0, ns), col0, ns)]


# ------------------------------------------------------------------------------------------------------------------
# backward: float64 sums, the number of terms and the sum of their magnitudes per element
# ------------------------------------------------------------------------------------------------------------------
def _rows_add(acc, s, g):
    """acc[s[i]] += g[i] for every i (repeated s allowed): rows grouped by a stable sort, each group summed at once"""
    if s.size == 0:
        return
    o = np.argsort(s, kind="stable")
    ss = s[o]
    starts = np.nonzero(np.concatenate([[True], ss[1:] != ss[:-1]]))[0]
    acc[ss[starts]] += np.add.reduceat(g[o], starts, axis=0)


def max_pool_bwd_ref(dy, arg, inds, ns, add=None):
    """(dx [ns, c] float64, n [ns, c] int64, sabs [ns, c] float64): dx[s, ch] = sum of dy[q, ch] over the pairs (q, col)
    with inds[q, col] == s and arg[q, ch] == col (+ add[s, ch]); n counts those pairs, sabs sums |dy| (+ |add|)"""
    dy = np.asarray(dy, np.float64)
    arg = np.asarray(arg)
    inds = np.asarray(inds)
    nq, h = inds.shape
    c = dy.shape[1]
    dx = np.zeros((ns, c))
    n = np.zeros((ns, c), np.int64)
    sabs = np.zeros((ns, c))
    live = _live(inds, ns)
    for col in range(h):
        rows = np.nonzero(live[:, col])[0]
        if rows.size == 0:
            continue
        hit = arg[rows] == col                               # [rows, c]
        if not hit.any():
            continue
        s = inds[rows, col]
        g = np.where(hit, dy[rows], 0.0)
        _rows_add(dx, s, g)
        _rows_add(n, s, hit.astype(np.int64))
        _rows_add(sabs, s, np.abs(g))
    if add is not None:
        a = np.asarray(add, np.float64)
        dx += a
        sabs += np.abs(a)
    return dx, n, sabs


def closest_pool_bwd_ref(dy, inds, ns):
    """(dx, n, sabs) as above: dx[s] = sum of dy[q] over the queries with inds[q, 0] == s"""
    dy = np.asarray(dy, np.float64)
    col0 = np.asarray(inds)[:, 0]
    c = dy.shape[1]
    rows = np.nonzero(_live(col0, ns))[0]
    dx = np.zeros((ns, c))
    sabs = np.zeros((ns, c))
    _rows_add(dx, col0[rows], dy[rows])
    _rows_add(sabs, col0[rows], np.abs(dy[rows]))
    cnt = np.bincount(col0[rows], minlength=ns)[:ns].astype(np.int64) if rows.size else np.zeros(ns, np.int64)
    return dx, np.broadcast_to(cnt[:, None], (ns, c)).copy(), sabs


def bwd_bound(n, sabs, ref, bf16=False):
    """per-element tolerance of a backward sum (module docstring)"""
    tol = (np.asarray(n, np.float64) + C_TREE) * U * sabs
    if bf16:
        tol = tol * (1.0 + 2.0 ** -8) + 2.0 ** -8 * np.abs(ref)
    return tol


def violations(got, ref, tol):
    """boolean mask of the elements outside their bound (NaN counts as outside)"""
    return ~(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)) <= tol)


def describe(got, ref, tol, what):
    bad = violations(got, ref, tol)
    if not bad.any():
        return ""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    tol = np.broadcast_to(np.asarray(tol, np.float64), got.shape)
    lines = ["%s: %d of %d elements outside the bound" % (what, int(bad.sum()), bad.size)]
    for t in np.argwhere(bad)[:5]:
        t = tuple(t)
        lines.append("  at %s: got %.9g ref %.9g |diff| %.3g tol %.3g" % (t, got[t], ref[t], abs(got[t] - ref[t]), tol[t]))
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------------------------
# transposed table
# ------------------------------------------------------------------------------------------------------------------
def transposed_table_ref(inds, ns):
    """(offsets [ns + 2] int64, pairs int64): exclusive scan of the per-support pair counts; every list ascending.  Slot ns
    (the shadow list) is empty -- shadow pairs are not tabulated -- so offsets[ns + 1] == offsets[ns] == len(pairs)"""
    flat = np.asarray(inds).reshape(-1)
    ids = np.nonzero(_live(flat, ns))[0]
    s = flat[ids]
    counts = np.bincount(s, minlength=ns + 1)[:ns + 1] if ids.size else np.zeros(ns + 1, np.int64)
    offsets = np.zeros(ns + 2, np.int64)
    offsets[1:] = np.cumsum(counts)
    pairs = ids[np.argsort(s, kind="stable")]                # ids ascend, the sort is stable: every list ascending
    return offsets, pairs.astype(np.int64)
