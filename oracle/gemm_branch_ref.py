"""oracle/gemm_branch_ref.py -- TEST INFRASTRUCTURE ONLY.

Float64 references and per-element error bounds for the dense products (tests/test_gemm_branches_*.py): the xb
products with their whole epilogue menu, dW = X^T dY, and the activation backward with column sums.

Reference epilogue (the kernels' order; weasal_amd/csrc/gemm_xb.hip)
  1. v = X @ B, + bias[col], + residual: residual[r] or, gathered, residual[rrows[r * rld]] (indices outside [0, rn):
     the shadow row, adds nothing);
  2. LeakyReLU(slope);
  3. dropout: keep = hash(seed, row * dn + col) >= threshold (`drop_keep`: a numpy replay of ws_drop_hash /
     ws_drop_args in ws_common.h, splitmix64 on uint64, threshold min(floor(p 2^32), 2^32 - 1)), v * scale with
     scale = 1.0f / (1.0f - p) computed in f32;
  4. the LeakyReLU' gate: v * (gate_y > 0 ? 1 : gate_slope), strictly, so 0 and -0.0 take the slope;
  5. the byte mask: mask ? v * mscale : 0.
  Every decision (dropout bits, gate sign, mask byte) depends on inputs only, so both sides take it the same way.

Error model (u = 2^-24; first order in u).  Never a fraction of the tensor's maximum.
  xb products:  |got - ref| <= (L + c) u (|X| @ |B| + |bias| + |res|) * F
    L  the longest chain of additions of the kernel: k for gemm_xb_kernel (MFMA k-steps), for gemm_xb_shallow_kernel
       (a sequential fmaf) and for un-split gemm_xb2; 32 csplit + splits for split gemm_xb2 (each layer's chain, then
       the fixed-order sum of the layers in splitk_epilogue_kernel).
    c  = 8: the epilogue's roundings -- bias and residual additions (either order: xb_rows_epilogue and the shallow
       kernel add residual then bias, gemm_xb_kernel and splitk_epilogue_kernel bias then residual; the model counts
       two additions and pins neither order), the slope, dropout scale, gate slope and mask scale products.
    F  = max(1, |slope|) [act] * scale [dropout] * max(1, |gate_slope|) [gate] * |mscale| [mask]: the factors the
       error of v is multiplied by on its way out.
    LeakyReLU near zero needs no rule of its own: the function is continuous and Lipschitz with constant
    max(1, |slope|), so where v and its reference straddle 0 the outputs differ by at most that constant times the
    error of v -- inside the bound.
  xty products (dW):  |got - ref| <= (L + 2) u (|X|^T @ |Y|)
    L = rows of one chunk (the serial MFMA chain of a row group, an upper bound) + 4 (row groups summed through LDS)
        + chunks (reduce_partials: sequential within a group, wide form fully sequential) + 8 (the 8-group tree).
    bf16 operands: the products of two bf16 values are exact in f32; only the sums round (the same L).
  act_bwd_colsum:  dz = gate(drop(dy)) rounds at most twice (scale, slope): |got - ref| <= 3 u |ref|.  The column sums:
    (chunk + chunks + 8 + 3) u sum_r |dz[r, col]| (row lanes within a chunk, the lanes through LDS, the chunks).
  bf16 outputs: inputs are rounded to bf16 before either side sees them; the kernel rounds its f32 result r once at the
    store (round to nearest even: <= 2^-8 |r|, and |r| <= |ref| + the f32 bound): f32 bound * (1 + 2^-8) + 2^-8 |ref|.
    (A bf16 dz feeding the sums: each term carries that rounding, + 2^-8 sum |dz|.)
"""
import numpy as np

U = 2.0 ** -24
C_EPI = 8.0


# ------------------------------------------------------------------------------------------------------------------
# dropout bits (ws_common.h: ws_drop_hash, ws_drop_args)
# ------------------------------------------------------------------------------------------------------------------
def drop_hash(seed, idx):
    """splitmix64 finaliser of seed + idx * golden, upper 32 bits (uint64 arithmetic, wrapping)"""
    with np.errstate(over="ignore"):
        i = np.asarray(idx, np.uint64)
        z = np.uint64(seed) + i * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint64)


def drop_args(p):
    """(threshold, scale): threshold = min(floor(p 2^32), 2^32 - 1) from the f32 p, scale = 1.0f / (1.0f - p) in f32"""
    p32 = np.float32(p)
    t = float(p32) * 4294967296.0
    thr = 4294967295 if t >= 4294967295.0 else int(t)
    scale = np.float32(1.0) / (np.float32(1.0) - p32)
    return thr, float(scale)


def drop_keep(seed, p, rows, cols, dn):
    """[rows, cols] bool: keep bit of element (r, c) at index r * dn + c"""
    thr, _ = drop_args(p)
    idx = np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(dn) + np.arange(cols, dtype=np.uint64)[None, :]
    return drop_hash(seed, idx) >= np.uint64(thr)


# ------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------
def gathered(residual, m, rrows=None, rld=1, rn=None):
    """[m, n] float64 residual rows of the output rows (zeros for the shadow row); residual None -> None"""
    if residual is None:
        return None
    res = np.asarray(residual, np.float64)
    if rrows is None:
        return res[:m]
    rn = res.shape[0] if rn is None else rn
    idx = np.asarray(rrows).reshape(-1)[::rld][:m]
    live = (idx >= 0) & (idx < rn)
    out = np.zeros((m, res.shape[1]))
    out[live] = res[idx[live]]
    return out


def xb_gates(v, m, n, act=False, slope=0.1, drop=None, gate_y=None, gate_slope=0.1, mask=None, mscale=1.0):
    """steps 2-5 of the epilogue on float64 v [m, n]; drop = (p, seed, dn)"""
    if act:
        v = np.where(v > 0, v, v * slope)
    if drop is not None:
        p, seed, dn = drop
        keep = drop_keep(seed, p, m, n, dn)
        v = np.where(keep, v * drop_args(p)[1], 0.0)
    if gate_y is not None:
        v = v * np.where(np.asarray(gate_y, np.float64)[:m, :n] > 0, 1.0, gate_slope)
    if mask is not None:
        v = np.where(np.asarray(mask)[:m, :n] != 0, v * mscale, 0.0)
    return v


def xb_factor(act=False, slope=0.1, drop=None, gate_y=None, gate_slope=0.1, mask=None, mscale=1.0):
    f = 1.0
    if act:
        f *= max(1.0, abs(slope))
    if drop is not None:
        f *= drop_args(drop[0])[1]
    if gate_y is not None:
        f *= max(1.0, abs(gate_slope))
    if mask is not None:
        f *= abs(mscale)
    return f


def xb_ref(x, b, bias=None, res=None, **gates):
    """the whole epilogue in float64; x [m, k], b [k, n] (the logical matrix), res = gathered(...) rows"""
    x = np.asarray(x, np.float64)
    b = np.asarray(b, np.float64)
    m, n = x.shape[0], b.shape[1]
    v = x @ b
    if bias is not None:
        v = v + np.asarray(bias, np.float64)[None, :n]
    if res is not None:
        v = v + res
    return xb_gates(v, m, n, **gates)


def xb_bound(x, b, L, bias=None, res=None, ref=None, bf16_out=False, **gates):
    """per-element tolerance [m, n] of an xb product (module docstring)"""
    M = np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(b, np.float64))
    if bias is not None:
        M = M + np.abs(np.asarray(bias, np.float64))[None, :M.shape[1]]
    if res is not None:
        M = M + np.abs(res)
    tol = (L + C_EPI) * U * M * xb_factor(**gates)
    if bf16_out:
        tol = tol * (1.0 + 2.0 ** -8) + 2.0 ** -8 * np.abs(ref)
    return tol


def xb_chain(k, splits=1, csplit=None):
    """L of the module docstring"""
    return 32 * csplit + splits if splits > 1 else k


def xb_zero_rows_f32(bias, res, n, act=False, slope=0.1, drop=None, gate_y=None, gate_slope=0.1, mask=None, mscale=1.0,
                     rows=None):
    """what an all-zero row of x must give, exactly, replayed in f32: (0 + res) + bias (both orders give the same bits:
    0 + r = r), then the f32 epilogue; rows = the row indices (for the dropout / gate / mask of those rows)"""
    rows = np.asarray(rows)
    v = np.zeros((rows.size, n), np.float32)
    if res is not None:
        v = v + np.asarray(res, np.float32)
    if bias is not None:
        v = (v + np.asarray(bias, np.float32)[None, :n]).astype(np.float32)
    if act:
        v = np.where(v > 0, v, v * np.float32(slope)).astype(np.float32)
    if drop is not None:
        p, seed, dn = drop
        thr, sc = drop_args(p)
        idx = rows.astype(np.uint64)[:, None] * np.uint64(dn) + np.arange(n, dtype=np.uint64)[None, :]
        v = np.where(drop_hash(seed, idx) >= np.uint64(thr), v * np.float32(sc), np.float32(0)).astype(np.float32)
    if gate_y is not None:
        v = (v * np.where(np.asarray(gate_y)[rows, :n] > 0, np.float32(1), np.float32(gate_slope))).astype(np.float32)
    if mask is not None:
        v = np.where(np.asarray(mask)[rows, :n] != 0, v * np.float32(mscale), np.float32(0)).astype(np.float32)
    return v


def xty_ref(x, y):
    return np.asarray(x, np.float64).T @ np.asarray(y, np.float64)


def xty_bound(x, y, chunk, chunks):
    M = np.abs(np.asarray(x, np.float64)).T @ np.abs(np.asarray(y, np.float64))
    return (chunk + 4 + chunks + 8 + 2) * U * M


def colsum_ref(dy, y=None, slope=0.1, drop=None):
    """(dz, colsum) in float64: dz = LeakyReLU'(y) * dropout_bwd(dy) (y None: dz = dropout_bwd(dy)); drop = (p, seed, dn)"""
    g = np.asarray(dy, np.float64)
    m, n = g.shape
    if drop is not None:
        p, seed, dn = drop
        g = np.where(drop_keep(seed, p, m, n, dn), g * drop_args(p)[1], 0.0)
    if y is not None:
        g = np.where(np.asarray(y, np.float64)[:m, :n] > 0, g, g * slope)
    return g, g.sum(0)


def colsum_bounds(dz_ref, chunk, chunks, bf16_dz=False):
    """(tol of dz [m, n], tol of the column sums [n])"""
    a = np.abs(dz_ref)
    tdz = 3 * U * a * (1.0 + 2.0 ** -8) + (2.0 ** -8 * a if bf16_dz else 0.0)
    tcs = (chunk + chunks + 8 + 3) * U * a.sum(0) + ((2.0 ** -8 + 3 * U) * a.sum(0) if bf16_dz else 0.0)
    return tdz, tcs


# ------------------------------------------------------------------------------------------------------------------
# checks (the form of oracle/kpconv_branch_ref.py)
# ------------------------------------------------------------------------------------------------------------------
def violations(got, ref, tol):
    """boolean mask of the elements outside their bound (NaN counts as outside)"""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    return ~(np.abs(got - ref) <= tol)


def describe(got, ref, tol, what):
    bad = violations(got, ref, tol)
    if not bad.any():
        return ""
    idx = np.argwhere(bad)[:5]
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    tol = np.broadcast_to(np.asarray(tol, np.float64), got.shape)
    lines = ["%s: %d of %d elements outside the bound" % (what, int(bad.sum()), bad.size)]
    for t in idx:
        t = tuple(t)
        lines.append("  at %s: got %.9g ref %.9g |diff| %.3g tol %.3g" % (t, got[t], ref[t], abs(got[t] - ref[t]), tol[t]))
    return "\n".join(lines)


def worst_ratio(got, ref, tol):
    """max |got - ref| / tol over the elements with tol > 0 (0 when none)"""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    tol = np.broadcast_to(np.asarray(tol, np.float64), got.shape)
    live = tol > 0
    return float((np.abs(got - ref)[live] / tol[live]).max()) if live.any() else 0.0
