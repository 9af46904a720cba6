"""oracle/kpconv_branch_ref.py -- TEST INFRASTRUCTURE ONLY.

Float64 reference and per-element error bounds for the KPConv gather (tests/test_kpconv_branches_*.py).

Geometry without decision flips
  Points lie on a 2^-6 lattice; kernel points (rigid and deformed) on the same lattice shifted by 2^-7 per axis.  Every
  neighbour offset n - kp then has components that are odd multiples of 2^-7 (never 0: no sqrt(0) gradient), and with
  coordinates below 2^4 every squared distance has at most 22 significant bits: it is exact in f32.  `extent_margin`
  checks that no squared distance lies within 1e-6 relative of extent^2, so the in-range test, the linear clamp, the
  `closest` arg-min and its exact ties decide the same way in f32 and in float64.

Error model (u = 2^-24; first order in u)
  wf[q,k,c] = mod[q,k] * sum_h w(q,h,k) x[inds[q,h], c].  With  M = sum_h |w| |x| |mod|  and  M1 = sum_{h real} |x|
  (both from the same oracle on |x|; influence forced to constant, no filter, for M1):
      |got - ref| <= (h + c1) u M + c2 u M1 * max(1, |mod|)      [+ 2^-8 |ref| for bf16 rows]
  * h: at most h non-zero products are summed in some order (fmaf chains, MFMA k-steps, partial rows added back, a
    shuffle tree): each addition rounds once, relative to a partial sum bounded by M.
  * c1: RELATIVE error of one weight and the products after it, in units of u.  constant: w = 1 exact; 2 for the
    modulation product and the final store.  gaussian: w = exp(t), t = -d2 / (2 sigma^2 + 1e-9) computed in f32
    (0.3f is 0.67 u off 0.3, three roundings of the denominator, the division: <= 8 u relative on t), then
    __expf = v_exp_f32(t log2 e) (one more rounding on t log2 e, 1 ulp = 2 u on the result): <= (9 |t| + 3) u, so
    c1 = 10 t_max + 6 with t_max the largest |t| of the case.
  * c2: ABSOLUTE error of a linear weight w = max(1 - sqrt(d2) * (1 / extent), 0), where w > 0 means s = sqrt(d2) /
    extent <= 1: 1/extent and v_sqrt_f32 within 1 ulp (2 u) each, one rounding of the product, so s is off by <= 5 u;
    1 - s is exact for s >= 1/2 (Sterbenz) and rounds once (<= u, relative to w <= 1) otherwise: <= 6 u -> c2 = 8.
    Where w is small its relative error is large; the absolute error times |x| summed over the row is what M1 bounds.
  * bf16 rows: inputs are rounded to bf16 before either side sees them; the kernel rounds its f32 result once when it
    stores the row: half an ulp of 8 significant bits, <= 2^-8 |result|, taken as 2^-8 |ref|.  (Two bf16 results of
    the same sum, e.g. two summation orders, are two roundings apart: 2^-7.)
  dx[s,c] = sum over the incoming (query, column) pairs and kernel points of w mod dwf[q,k,c]: the same form with h
  replaced by the number of incoming products (K * incoming pairs, plus 6 for the shuffle tree over the entry slots).
  Geometry gradients (K6, linear influence): d deformed_kp[q,k] = sum_h dot_hk mod (kp - n_h) / (extent sd_hk)
  + d_min_d2 * 2 (kp - n*) with dot_hk = sum_c dwf[q,k,c] x[inds[q,h],c].  Each dot has ci products (ci u relative to
  dot_abs = sum_c |dwf| |x|), the coefficient a few roundings (sqrt, product, division, modulation: c1 = 8), the sum
  over h another h:  |err| <= (ci + h + c1) u Mg  with Mg the same sum over absolute values.  d modulations[q,k] =
  sum_h w dot: (ci + h + c1) u sum_h |w| dot_abs + c2 u sum_{h live} dot_abs.

Deformable fast path (MODE 2: ws_kpconv_gather_fwd_def / _bwd_x_def / _bwd_geom_def; kp4 = (x, y, z, modulation))
  The same formulas with three differences in how a term is evaluated; none of them moves a constant above.
  * forward and dx: the weight is  max(1 - v_sqrt(d2) * (1 / extent), 0) * mod  -- the modulation multiplies the influence
    before the product instead of the finished row.  1 / extent is a correctly rounded division (u), v_sqrt 1 ulp (2 u), the
    product u, 1 - s at most u: 5 u absolute on w <= 1, i.e. <= 5 u |mod| on the modulated weight, inside
    c2 max(1, |mod|) = 8 max(1, |mod|).  The product with mod rounds once (u, relative) where the generic kernel rounds the
    row once: c1 = 2 as before.  The number of additions per element is unchanged (h, or the incoming products).
  * geometry: sd = d2 * v_rsq(d2) replaces v_sqrt: v_rsq 1 ulp (2 u) and one product (u), 3 u relative on sd; with
    1 / extent (u), the product (u) and 1 - s (u): <= 6 u absolute on w <= c2 = 8 (d modulation = sum_h w dot, the
    unmodulated influence).
  * geometry: the coefficient of (n - kp) is  dot * (mod * (1 / extent)) * rs:  1 / extent u, the product with mod u, v_rsq
    2 u, two more products 2 u: 6 u relative <= c1 = 8; the fmaf into the running sum is one of the h additions, n - kp
    is exact on the lattice.  Where mod = 0 the coefficient is an exact 0, and so is the bound.
  min_d2: on a row with a real column every candidate of the minimum is a lattice distance, exact in f32; the tests keep
  the 4 u |ref| of the generic deformable rows.  On a row of shadow columns only the minimum is the shadow point's own
  distance, evaluated in f32 as  a = fl(1e6 - q)  (u, relative),  d = fl(a - kp)  (u, and a's error relative to d: |a| / |d|
  <= 1 + 4e-6 since |kp| < 2), so d is 2 u off; d * d 4 u + u; the sum of three non-negative squares two more additions:
  7 u (a contraction into fma only removes roundings) -> `min_d2_bound` takes 8 u |ref| there.  The d_min_d2 term of
  d kp, 2 g (kp - (s* - q)) at the arg-min column s*, is a, the subtraction and the rounding of the fmaf that adds it: 3 u
  relative to |kp| + |s* - q|, within the (h + 8) u that `geom_bounds` already grants it (h >= 1).
  Sorted-row cutoff (CUT): the columns it skips have 15 zero influences and cannot lower a minimum; the skipped terms are
  fmaf / MFMA steps with an exact 0 factor, and the lanes keep their columns: same summation split, results equal bit for
  bit to the walk without the cutoff.
"""
import numpy as np
import torch

from oracle.kpconv_ref import kpconv_gather_ref

U = 2.0 ** -24
STEP = 2.0 ** -6          # point lattice
KP_SHIFT = 2.0 ** -7      # kernel points sit half a lattice step off it (per axis)
C2_LINEAR = 8.0           # absolute error of one linear weight, units of u (module docstring)


# ------------------------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------------------------
def lattice_cloud(rng, n, half):
    """n points on the 2^-6 lattice in the cube [-half, half]^3, f32"""
    m = int(half / STEP)
    return (rng.integers(-m, m + 1, size=(n, 3)) * STEP).astype(np.float32)


def lattice_kernel(rng, k, reach):
    """k rigid kernel points within `reach` of the origin: lattice + 2^-7 per axis, f32"""
    m = int(reach / STEP)
    out = []
    while len(out) < k:
        c = rng.integers(-m, m + 1, size=3) * STEP + KP_SHIFT
        if (c.astype(np.float64) ** 2).sum() <= reach * reach:
            out.append(c)
    return np.asarray(out, np.float32)


def lattice_deformed(rng, kp, nq, jitter):
    """per-query deformed kernel points [nq, K, 3]: kp moved by whole lattice steps (stays 2^-7 off the lattice)"""
    m = max(1, int(jitter / STEP))
    return (kp[None].astype(np.float64) + rng.integers(-m, m + 1, size=(nq,) + kp.shape) * STEP).astype(np.float32)


def brute_rows(q, s, radius, h):
    """[nq, h] int64: the h nearest supports of each query that lie within `radius`, nearest first (index order on
    ties), padded with the shadow index ns"""
    q64, s64 = q.astype(np.float64), s.astype(np.float64)
    ns = s.shape[0]
    out = np.full((q.shape[0], h), ns, np.int64)
    for a in range(0, q.shape[0], 512):
        d2 = ((q64[a:a + 512, None, :] - s64[None]) ** 2).sum(-1)
        cand = np.argpartition(d2, h - 1, axis=1)[:, :h] if h < ns else np.tile(np.arange(ns), (d2.shape[0], 1))
        cd = np.take_along_axis(d2, cand, 1)
        srt = np.lexsort((cand, cd), axis=1)                                   # by distance, then index
        order = np.take_along_axis(cand, srt, 1)
        dd = np.take_along_axis(cd, srt, 1)
        out[a:a + 512, :order.shape[1]] = np.where(dd < radius * radius, order, ns)
    return out


def extent_margin(q, s, inds, kp, extent, deformed=None):
    """smallest | d2 / extent^2 - 1 | over every real (query, neighbour, kernel point) triple (float64)"""
    e2 = float(np.float32(extent)) ** 2
    s_pad = np.concatenate([s.astype(np.float64), np.full((1, 3), 1e6)])
    worst = np.inf
    for a in range(0, q.shape[0], 256):
        ii = inds[a:a + 256]
        n = s_pad[ii] - q[a:a + 256, None, :].astype(np.float64)
        k = deformed[a:a + 256, None].astype(np.float64) if deformed is not None else kp.astype(np.float64)[None, None]
        d2 = (((n[:, :, None, :] - k) ** 2).sum(-1))[ii < s.shape[0]]
        if d2.size:
            worst = min(worst, float(np.abs(d2 / e2 - 1.0).min()))
    return worst


def gaussian_tmax(q, s, inds, kp, extent, deformed=None):
    """largest |t| = d2 / (2 sigma^2) over the real triples of a case (gaussian influence)"""
    sig = float(np.float32(extent)) * 0.3
    s_pad = np.concatenate([s.astype(np.float64), np.full((1, 3), np.nan)])
    best = 0.0
    for a in range(0, q.shape[0], 256):
        ii = inds[a:a + 256]
        n = s_pad[ii] - q[a:a + 256, None, :].astype(np.float64)
        k = deformed[a:a + 256, None].astype(np.float64) if deformed is not None else kp.astype(np.float64)[None, None]
        d2 = ((n[:, :, None, :] - k) ** 2).sum(-1)
        d2 = d2[ii < s.shape[0]]
        if d2.size:
            best = max(best, float(d2.max()) / (2 * sig * sig))
    return best


def closest_tie_count(q, s, inds, kp, deformed=None):
    """number of real (query, neighbour) pairs whose nearest kernel point is not unique"""
    s_pad = np.concatenate([s.astype(np.float64), np.full((1, 3), 1e6)])
    ties = 0
    for a in range(0, q.shape[0], 256):
        ii = inds[a:a + 256]
        n = s_pad[ii] - q[a:a + 256, None, :].astype(np.float64)
        k = deformed[a:a + 256, None].astype(np.float64) if deformed is not None else kp.astype(np.float64)[None, None]
        d2 = ((n[:, :, None, :] - k) ** 2).sum(-1)
        m = d2.min(-1, keepdims=True)
        ties += int((((d2 == m).sum(-1) > 1) & (ii < s.shape[0])).sum())
    return ties


# ------------------------------------------------------------------------------------------------------------------
# float64 reference (kpconv_gather_ref in chunks of queries)
# ------------------------------------------------------------------------------------------------------------------
def _t(a):
    return torch.as_tensor(np.asarray(a)).to(torch.float64) if not isinstance(a, torch.Tensor) else a.to(torch.float64)


def _chunk(h, k, ci):
    per_query = 8 * (h * k * 12 + h * ci + 2 * k * ci + h * k * 4)
    return int(max(16, min(4096, 3e8 // max(per_query, 1))))


def ref_forward(x, q, s, inds, kp, extent, influence="linear", aggregation="sum", deformed=None, mod=None):
    """(wf [nq,K,ci], min_d2 [nq,K] or None) in float64 from the f32 values"""
    x, q, s, kp = _t(x), _t(q), _t(s), _t(kp)
    inds = torch.as_tensor(np.asarray(inds)).long()
    dk = _t(deformed) if deformed is not None else None
    md = _t(mod) if mod is not None else None
    nq, h = inds.shape
    ext = float(np.float32(extent))
    step = _chunk(h, kp.shape[0], x.shape[1])
    wf, mn = [], []
    for a in range(0, nq, step):
        b = min(nq, a + step)
        w, m = kpconv_gather_ref(x, q[a:b], s, inds[a:b], kp, ext, influence, aggregation,
                                 dk[a:b] if dk is not None else None, md[a:b] if md is not None else None)
        wf.append(w)
        if m is not None:
            mn.append(m)
    return torch.cat(wf).numpy(), (torch.cat(mn).numpy() if mn else None)


def ref_backward(x, dwf, q, s, inds, kp, extent, influence="linear", aggregation="sum", deformed=None, mod=None, dmin=None):
    """float64 autograd of  sum(wf * dwf) + sum(min_d2 * dmin)  -> (dx, d deformed_kp or None, d modulations or None)"""
    xl = _t(x).clone().requires_grad_(True)
    q, s, kp, dwf = _t(q), _t(s), _t(kp), _t(dwf)
    inds = torch.as_tensor(np.asarray(inds)).long()
    nq, h = inds.shape
    ext = float(np.float32(extent))
    dk = _t(deformed) if deformed is not None else None
    md = _t(mod) if mod is not None else None
    dm = _t(dmin) if dmin is not None else None
    step = _chunk(h, kp.shape[0], x.shape[1])
    gk, gm = [], []
    for a in range(0, nq, step):
        b = min(nq, a + step)
        dkc = dk[a:b].clone().requires_grad_(True) if dk is not None else None
        mdc = md[a:b].clone().requires_grad_(True) if md is not None else None
        w, m = kpconv_gather_ref(xl, q[a:b], s, inds[a:b], kp, ext, influence, aggregation, dkc, mdc)
        loss = (w * dwf[a:b]).sum()
        if dm is not None and m is not None:
            loss = loss + (m * dm[a:b]).sum()
        loss.backward()
        if dkc is not None:
            gk.append(dkc.grad if dkc.grad is not None else torch.zeros_like(dkc))
        if mdc is not None:
            gm.append(mdc.grad if mdc.grad is not None else torch.zeros_like(mdc))
    return (xl.grad.numpy(), torch.cat(gk).numpy() if gk else None, torch.cat(gm).numpy() if gm else None)


# ------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------
def weight_constants(influence, tmax=0.0):
    """(c1, c2) of the module docstring for an influence"""
    if influence == "linear":
        return 2.0, C2_LINEAR
    if influence == "gaussian":
        return 10.0 * tmax + 6.0, 0.0
    return 2.0, 0.0


def fwd_bound(x, q, s, inds, kp, extent, influence, aggregation, deformed=None, mod=None, tmax=0.0, ref=None, bf16=False):
    """per-element tolerance [nq,K,ci] of wf (module docstring)"""
    h = np.asarray(inds).shape[1]
    ax = np.abs(np.asarray(x, np.float64))
    am = np.abs(np.asarray(mod, np.float64)) if mod is not None else None
    M, _ = ref_forward(ax, q, s, inds, kp, extent, influence, aggregation, deformed, am)
    M1, _ = ref_forward(ax, q, s, inds, kp, extent, "constant", "sum")
    c1, c2 = weight_constants(influence, tmax)
    tol = (h + c1) * U * M + c2 * U * M1 * max(1.0, float(am.max()) if am is not None and am.size else 1.0)
    if bf16:
        tol = tol + 2.0 ** -8 * np.abs(ref)
    return tol


def incoming_products(inds, ns, k=15):
    """K * (number of (query, column) pairs pointing at each support) + 6: the products summed into one dx row"""
    ii = np.asarray(inds).reshape(-1)
    cnt = np.bincount(ii[ii < ns], minlength=ns)[:ns]
    return k * cnt.astype(np.float64) + 6.0


def dx_bound(dwf, q, s, inds, kp, extent, influence, aggregation, deformed=None, mod=None, tmax=0.0, ref=None, bf16=False,
             x_shape=None):
    """per-element tolerance [ns, ci] of dx (module docstring).  All weights are >= 0 (modulations too, in these
    tests), so the reference backward on |dwf| is the sum of the absolute products."""
    ns = s.shape[0]
    adw = np.abs(np.asarray(dwf, np.float64))
    am = np.abs(np.asarray(mod, np.float64)) if mod is not None else None
    zeros = np.zeros(x_shape, np.float64)
    M, _, _ = ref_backward(zeros, adw, q, s, inds, kp, extent, influence, aggregation, deformed, am)
    M1, _, _ = ref_backward(zeros, adw, q, s, inds, kp, extent, "constant", "sum")
    c1, c2 = weight_constants(influence, tmax)
    n = incoming_products(inds, ns, kp.shape[0])[:, None]
    tol = (n + c1) * U * M + c2 * U * M1 * max(1.0, float(am.max()) if am is not None and am.size else 1.0)
    if bf16:
        tol = tol + 2.0 ** -8 * np.abs(ref)
    return tol


def geom_bounds(x, dwf, q, s, inds, deformed, mod, extent, influence, aggregation, dmin=None):
    """per-element tolerances (d deformed_kp [nq,K,3], d modulations [nq,K]) of the K6 geometry backward (module
    docstring), float64, from the absolute values of every term"""
    x = np.asarray(x, np.float64)
    dwf = np.asarray(dwf, np.float64)
    inds = np.asarray(inds)
    nq, h = inds.shape
    ns, ci = x.shape
    ext = float(np.float32(extent))
    kq = np.asarray(deformed, np.float64)
    k = kq.shape[1]
    md = np.abs(np.asarray(mod, np.float64)) if mod is not None else np.ones((nq, k))
    s_pad = np.concatenate([np.asarray(s, np.float64), np.full((1, 3), 1e6)])
    x_pad = np.concatenate([np.abs(x), np.zeros((1, ci))])
    e2 = ext * ext
    sig2 = 2 * (ext * 0.3) ** 2 + 1e-9
    tol_k = np.zeros((nq, k, 3))
    tol_m = np.zeros((nq, k))
    step = max(1, int(2e7 // max(1, h * k * (ci + 8))))
    for a in range(0, nq, step):
        b = min(nq, a + step)
        ii = inds[a:b]
        n = s_pad[ii] - np.asarray(q, np.float64)[a:b, None, :]                  # [B,H,3]
        diff = n[:, :, None, :] - kq[a:b, None]                                 # [B,H,K,3]
        sq = (diff ** 2).sum(-1)                                                # [B,H,K]
        real = (ii < ns)[:, :, None]
        if influence == "linear":
            w = np.maximum(1 - np.sqrt(sq) / ext, 0.0)
            fac = np.where(w > 0, 1.0 / (ext * np.sqrt(sq)), 0.0)
        elif influence == "gaussian":
            w = np.exp(-sq / sig2)
            fac = w * 2.0 / sig2
        else:
            w = np.ones_like(sq)
            fac = np.zeros_like(sq)
        if aggregation == "closest":
            one = np.zeros_like(sq)
            np.put_along_axis(one, sq.argmin(-1)[..., None], 1.0, -1)
            w, fac = w * one, fac * one
        keep = (sq < e2).any(-1, keepdims=True)
        live = (w != 0) & real & keep
        w, fac = np.where(live, w, 0.0), np.where(live, fac, 0.0)
        dot_abs = np.einsum("bkc,bhc->bhk", np.abs(dwf[a:b]), x_pad[ii])          # [B,H,K]
        c1 = 8.0
        if influence == "gaussian":
            c1 += 10.0 * float((sq[live] / sig2).max(initial=0.0))
        mg = np.einsum("bhk,bhkd->bkd", dot_abs * fac, np.abs(diff)) * md[a:b, :, None]
        tol_k[a:b] = (ci + h + c1) * U * mg
        tol_m[a:b] = (ci + h + c1) * U * (w * dot_abs).sum(1) + C2_LINEAR * U * (live * dot_abs).sum(1)
        if dmin is not None:
            arg = sq.argmin(1)                                                  # first column wins, as torch.min
            nstar = np.take_along_axis(n[:, :, None, :].repeat(k, 2), arg[:, None, :, None], 1)[:, 0]   # [B,K,3]
            gmin = np.abs(np.asarray(dmin, np.float64)[a:b])[..., None]
            tol_k[a:b] += (h + 8.0) * U * 2 * gmin * (np.abs(kq[a:b]) + np.abs(nstar))
    return tol_k, tol_m


def _offsets(q, s, inds, a, b):
    """neighbour offsets [B,H,3] of queries a..b in float64 (shadow index -> the point (1e6, 1e6, 1e6))"""
    s_pad = np.concatenate([np.asarray(s, np.float64), np.full((1, 3), 1e6)])
    return s_pad[np.asarray(inds)[a:b]] - np.asarray(q, np.float64)[a:b, None, :]


def min_d2_bound(ref_min, q, s, inds, deformed):
    """per-element tolerance [nq,K] of min_d2 (module docstring): 4 u |ref| where the arg-min column is a real neighbour,
    8 u |ref| where it is a shadow column"""
    inds = np.asarray(inds)
    ns = np.asarray(s).shape[0]
    kq = np.asarray(deformed, np.float64)
    shadow = np.zeros(kq.shape[:2], bool)
    for a in range(0, inds.shape[0], 128):
        b = min(inds.shape[0], a + 128)
        sq = ((_offsets(q, s, inds, a, b)[:, :, None, :] - kq[a:b, None]) ** 2).sum(-1)        # [B,H,K]
        arg = sq.argmin(1)                                                                     # [B,K]
        shadow[a:b] = np.take_along_axis(inds[a:b], arg, 1) >= ns
    return np.where(shadow, 8.0, 4.0) * U * np.abs(np.asarray(ref_min, np.float64))


def cutoff_counts(q, s, inds, deformed, extent):
    """what a sorted-row case holds (float64): (queries whose last column with a non-zero influence is >= 64,
    (query, kernel point) pairs whose min_d2 arg-min column is >= 64, queries whose first column is a real neighbour
    already beyond max |kp| + extent, queries whose walk ends inside the second 64-column chunk, ... inside the third).
    The walk of a query: the first chunk in full, then up to the first column farther from the query than
    R = 1.0001 max(max |kp| + extent, max_k (sqrt(min d2[k] over the first chunk) + |kp_k|)); it ends inside a chunk when
    that column is a real neighbour and neither the first nor past the last column of the chunk (the cutoff, not the end of
    the row or of a chunk, ends it)."""
    inds = np.asarray(inds)
    ns = np.asarray(s).shape[0]
    ext = float(np.float32(extent))
    kq = np.asarray(deformed, np.float64)
    last_far = arg_far = first_beyond = second = third = 0
    cols = np.arange(inds.shape[1])
    for a in range(0, inds.shape[0], 128):
        b = min(inds.shape[0], a + 128)
        n = _offsets(q, s, inds, a, b)
        sq = ((n[:, :, None, :] - kq[a:b, None]) ** 2).sum(-1)                                  # [B,H,K]
        real = inds[a:b] < ns
        infl = ((sq < ext * ext).any(-1)) & real                                               # [B,H]
        last = np.where(infl, cols[None], -1).max(1)
        last_far += int((last >= 64).sum())
        arg_far += int((sq.argmin(1) >= 64).sum())
        rk = np.sqrt((kq[a:b] ** 2).sum(-1))                                                    # [B,K]
        reach = rk.max(1) + ext
        dn = np.sqrt((n ** 2).sum(-1))                                                          # [B,H]
        first_beyond += int((real[:, 0] & (dn[:, 0] > reach)).sum())
        big = 1.0001 * np.maximum(reach, (np.sqrt(sq[:, :64].min(1)) + rk).max(1))
        beyond = (cols[None] >= 64) & ((dn > big[:, None]) | ~real)
        stop = np.where(beyond.any(1), beyond.argmax(1), inds.shape[1])
        ended = (stop < inds.shape[1]) & np.take_along_axis(real, np.minimum(stop, inds.shape[1] - 1)[:, None], 1)[:, 0]
        second += int((ended & (stop > 64) & (stop < 128)).sum())
        third += int((ended & (stop > 128) & (stop < 192)).sum())
    return last_far, arg_far, first_beyond, second, third


def worst_ratio(got, ref, tol):
    """(largest |got - ref| / tol over the elements, number of elements); an element with tol = 0 counts 0 when it is exact
    and inf otherwise"""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    tol = np.broadcast_to(np.asarray(tol, np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    return (float(ratio.max()) if ratio.size else 0.0), int(err.size)


def violations(got, ref, tol):
    """boolean mask of the elements outside their bound"""
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
    lines = ["%s: %d of %d elements outside the bound" % (what, int(bad.sum()), bad.size)]
    for t in idx:
        t = tuple(t)
        lines.append("  at %s: got %.9g ref %.9g |diff| %.3g tol %.3g" % (t, got[t], ref[t], abs(got[t] - ref[t]), tol[t]))
    return "\n".join(lines)
