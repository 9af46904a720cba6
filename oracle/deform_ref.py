"""oracle/deform_ref.py -- TEST INFRASTRUCTURE ONLY.

Float64 restatements and per-element error bounds for the element-wise ends of a deformable KPConv
(weasal_amd/csrc/deform.hip): ws_kpconv_deform_prepare / _bwd and ws_p2p_regularizer_fwd / _bwd.  The bounds follow the
roundings written in the kernels (u = 2^-24, first order in u), in the style of oracle/kpconv_branch_ref.py.

deform_prepare (offset features [n, 3K | 4K] -> kp4 [n, K, 4] = (x, y, z, modulation))
  position   v = fl(fl(off * extent) + kp): two roundings, no FMA (the kernel switches contraction off):
             |err| <= u |off extent| + u |v|.
  modulation m = 2 / (1 + __expf(-z)).  __expf(a) = v_exp_f32(a log2 e): the product a log2 e rounds once and log2 e is
             half an ulp off, together <= 2 u relative on t = a log2 e, which moves the result by 2 |t| u relative; v_exp_f32
             is good to 1 ulp (2 u): E = e^-z (1 + (2 |t| + 2) u).  1 + E rounds once (u), the division is correctly rounded
             (u; 2 u granted), the factor 2 is exact.  E enters 1 / (1 + E) with weight E / (1 + E) = 1 - m / 2:
             |err| <= m u (3 + (2 |z| log2 e + 2)(1 - m / 2)).
  kp_rmax    max over the launch of r = sqrtf((x x + y y) + z z) of the f32 positions: three squares (u each), two additions
             (2 u): 3 u relative on the sum, halved by the root, plus its rounding: 2.5 u.  The float64 maximum norm of the
             f32 positions the kernel wrote, times (1 -+ 4 u), bounds it on both sides.
  backward   d off[3k + c] = fl(g extent): u |ref|; with a second position gradient g = fl(g1 + g2) first: 2 u |ref|.
             d off[3K + k] = g_w m (1 - m / 2) with the f32 m the forward stored: 0.5 m exact, 1 - 0.5 m u, two products
             2 u: 3 u |ref|, plus what the forward error of m does to it: |g_w| |1 - m| tol(m).

p2p_regularizer (models/architectures.py:24-57: fitting, repulsive of one layer; loc = deformed_kp / extent)
  fitting    mean |min_d2 / extent^2|.  1 / fl(extent extent) 2 u, the product u: 3 u per term.  One thread adds the 15 terms
             of each of its points (n / (256 blocks) points, rounded up), a shuffle tree of 6 and 2 more additions close a
             workgroup in f32; the workgroups are added in double.  All terms are >= 0, so the sum of absolute terms is
             the result:  |err| <= (3 + adds + 1) u fitting,  adds = 15 ceil(n / (256 blocks)) + 8, + 1 for the store.
  repulsive  sum_i mean_n sum_{j != i} c_ij^2 / K,  c = min(d - repulse_extent, 0),  d = |loc_i - loc_j|.
             loc = fl(v fl(1 / extent)): 2 u relative.  dx = fl(l_j - l_i): |err| <= 2 u (|l_j| + |l_i|) + u |dx| =: e_x.  d: the
             component errors enter with weight |dx_c| / d <= 1, the squares, sums and the root add 3.5 u relative:
             e_d = e_x + e_y + e_z + 4 u d.  c: e_c = e_d + u |c|;  c^2: 2 |c| e_c + u c^2.  14 terms per i and the same
             reduction as the fitting term: (14 + adds + 1) u relative to the sum of the c^2.  The setup keeps every d
             1e-5 away from repulse_extent (e_d is below 1e-6 at these sizes), so the clamp decides alike on both sides.
  backward   d min_d2 = sign(min_d2) g_fit / (extent^2 n K): 1 / extent^2 2 u, product, division: 4 u; 6 u |ref| granted.
             d deformed_kp[n, i] = g_rep / (n K extent) sum_{j != i} f_ij (l_i - l_j),  f = 2 c / d (0 where c = 0):
             per term  2 (e_c |dx| / d + |c| e_d |dx| / d^2) + |f| e_x + 2 u |f dx|  (the division and the doubling), 14
             fmaf additions and the factor g_rep (4 u) with its product (u): (14 + 5) u relative to sum_j |f dx|.
"""
import numpy as np
import torch

U = 2.0 ** -24
K = 15
LOG2E = 1.4426950408889634


# ------------------------------------------------------------------------------------------------------------------
# deform_prepare
# ------------------------------------------------------------------------------------------------------------------
def prepare_ref(off, kernel_points, extent, modulated):
    """-> (kp4 [n,K,4] float64, tol [n,K,4]) from the f32 offset features, kernel points and the f32 extent"""
    off = np.asarray(off, np.float64)
    kp = np.asarray(kernel_points, np.float64)
    ext = float(np.float32(extent))
    n = off.shape[0]
    o = off[:, :3 * K].reshape(n, K, 3) * ext
    v = o + kp[None]
    kp4 = np.ones((n, K, 4))
    tol = np.zeros((n, K, 4))
    kp4[..., :3] = v
    tol[..., :3] = U * (np.abs(o) + np.abs(v))
    if modulated:
        z = off[:, 3 * K:]
        m = 2.0 / (1.0 + np.exp(-z))
        kp4[..., 3] = m
        tol[..., 3] = m * U * (3.0 + (2.0 * np.abs(z) * LOG2E + 2.0) * (1.0 - 0.5 * m))
    return kp4, tol


def prepare_torch(off, kernel_points, extent, modulated):
    """the forward in torch float64 (autograd): kp4 [n,K,4]"""
    n = off.shape[0]
    v = off[:, :3 * K].reshape(n, K, 3) * extent + kernel_points[None]
    m = 2.0 * torch.sigmoid(off[:, 3 * K:]) if modulated else torch.ones((n, K), dtype=off.dtype)
    return torch.cat([v, m[..., None]], -1)


def prepare_bwd_ref(off, d_kp4, d_dkp, extent, modulated, m_tol=None):
    """analytic gradient of sum(kp4 * d_kp4) + sum(kp4[..., :3] * d_dkp) w.r.t. the offset features
    -> (d_off [n, od] float64, tol [n, od]); m_tol: the forward tolerance of the modulation (prepare_ref)"""
    off = np.asarray(off, np.float64)
    g = np.asarray(d_kp4, np.float64)
    ext = float(np.float32(extent))
    n = off.shape[0]
    gp = g[..., :3] + (np.asarray(d_dkp, np.float64) if d_dkp is not None else 0.0)
    d_pos = (gp * ext).reshape(n, 3 * K)
    t_pos = (2.0 if d_dkp is not None else 1.0) * U * np.abs(d_pos)
    if not modulated:
        return d_pos, t_pos
    m = 2.0 / (1.0 + np.exp(-off[:, 3 * K:]))
    d_mod = g[..., 3] * m * (1.0 - 0.5 * m)
    t_mod = 3.0 * U * np.abs(d_mod) + np.abs(g[..., 3]) * np.abs(1.0 - m) * (m_tol if m_tol is not None else 0.0)
    return np.concatenate([d_pos, d_mod], 1), np.concatenate([t_pos, t_mod], 1)


# ------------------------------------------------------------------------------------------------------------------
# p2p regulariser
# ------------------------------------------------------------------------------------------------------------------
def regularizer_torch(deformed_kp, min_d2, extent, repulse_extent, others=None):
    """the torch twin of `regularizer_ref` (autograd): tensor [2] = (fitting, repulsive) in the broadcast [n, K, K] form of
    `_pairs`.  The partner of every pair is a constant (models/architectures.py:52 detaches it).  others: the points the
    partners are taken from (default: deformed_kp itself; given apart it makes the function whose plain derivative autograd
    returns, for gradcheck)"""
    n = min_d2.shape[0]
    fit = (min_d2 / (extent * extent)).abs().sum() / (n * K)
    loc = deformed_kp / extent
    partner = (loc if others is None else others / extent).detach()
    diff = loc[:, :, None, :] - partner[:, None, :, :]                         # [n, i, j, 3] = l_i - l_j
    eye = torch.eye(K, dtype=torch.bool)[None, :, :, None]
    # (the diagonal holds d = 0, whose root has no finite derivative: replaced before the root, masked after it)
    d = torch.where(eye, torch.ones_like(diff), diff).pow(2).sum(-1).sqrt()
    c = torch.where(eye[..., 0], torch.zeros_like(d), (d - repulse_extent).clamp(max=0.0))
    rep = c.pow(2).sum(2).abs().sum() / (n * K)
    return torch.stack([fit, rep])


def _adds(n):
    blocks = min(1024, max(1, -(-n // 256)))
    return 15 * (-(-n // (256 * blocks))) + 8


def _pairs(deformed_kp, extent, repulse_extent):
    """float64 pieces of the repulsive term: dx [n,K,K,3] = l_i - l_j, d, c, and the error terms e_x [n,K,K,3], e_d, e_c"""
    ext = float(np.float32(extent))
    loc = np.asarray(deformed_kp, np.float64) / ext
    al = np.abs(loc)
    dx = loc[:, :, None, :] - loc[:, None, :, :]
    d = np.sqrt((dx ** 2).sum(-1))
    c = np.minimum(d - float(np.float32(repulse_extent)), 0.0)
    off = ~np.eye(K, dtype=bool)[None]
    c = np.where(off, c, 0.0)
    e_x = 2 * U * (al[:, :, None, :] + al[:, None, :, :]) + U * np.abs(dx)
    e_d = e_x.sum(-1) + 4 * U * d
    e_c = e_d + U * np.abs(c)
    return dx, d, c, e_x, e_d, e_c, off


def repulse_margins(deformed_kp, extent, repulse_extent):
    """[n]: per point, the smallest | |loc_i - loc_j| - repulse_extent | over its pairs i != j"""
    dx, d, c, e_x, e_d, e_c, off = _pairs(deformed_kp, extent, repulse_extent)
    return np.where(off, np.abs(d - float(np.float32(repulse_extent))), np.inf).min((1, 2))


def regularizer_ref(deformed_kp, min_d2, extent, repulse_extent):
    """-> (out [2] float64, tol [2])"""
    ext = float(np.float32(extent))
    md = np.asarray(min_d2, np.float64)
    n = md.shape[0]
    fit = np.abs(md / (ext * ext)).sum() / (n * K)
    dx, d, c, e_x, e_d, e_c, off = _pairs(deformed_kp, extent, repulse_extent)
    rep = (c ** 2).sum() / (n * K)
    adds = _adds(n)
    t_fit = (3 + adds + 1) * U * fit
    t_rep = ((2 * np.abs(c) * e_c + U * c ** 2) * (c != 0)).sum() / (n * K) + (14 + adds + 1) * U * rep
    return np.array([fit, rep]), np.array([t_fit, t_rep])


def regularizer_bwd_ref(deformed_kp, min_d2, extent, repulse_extent, g):
    """analytic gradient of  g[0] fitting + g[1] repulsive  -> (d_deformed_kp, tol, d_min_d2, tol)"""
    ext = float(np.float32(extent))
    md = np.asarray(min_d2, np.float64)
    n = md.shape[0]
    g = np.asarray(g, np.float64)
    d_md = np.sign(md) * g[0] / (ext * ext * n * K)
    dx, d, c, e_x, e_d, e_c, off = _pairs(deformed_kp, extent, repulse_extent)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(c != 0, 2 * c / d, 0.0)
        dxd = np.where(d[..., None] > 0, np.abs(dx) / d[..., None], 0.0)
        cdd = np.where(d > 0, np.abs(c) / d, 0.0)
    live = (c != 0)[..., None]
    term = f[..., None] * dx                                                     # [n, i, j, 3]
    t_term = (2 * (e_c[..., None] * dxd + (cdd * e_d)[..., None] * dxd) + np.abs(f)[..., None] * e_x + 2 * U * np.abs(term)) * live
    scale = g[1] / (n * K * ext)
    d_kp = scale * term.sum(2)
    t_kp = np.abs(scale) * (t_term.sum(2) + 19 * U * np.abs(term).sum(2))
    return d_kp, t_kp, d_md, 6 * U * np.abs(d_md)
