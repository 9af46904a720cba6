"""oracle/kpconv_bf16_ref.py -- TEST INFRASTRUCTURE ONLY.

A float64 rounding replay of ONE deformable + modulated KPConv layer on bf16 feature rows (BASELINE config 5: linear
influence, sum aggregation; the deformable fast path of weasal_amd.blocks.KPConv.forward) and of its backward.  Every
value is carried in float64 and rounded to bf16 exactly where the HIP path stores a bf16 value, and nowhere else, so that
what is left between this replay and the GPU is fp32 accumulation order and the rare rounding tie it decides.  The
operator sequence is oracle.kpconv_ref.kpconv_gather_ref (models/blocks.py:278-367) plus the prepare step of
weasal_amd/blocks.py (unscaled * extent + kernel points, 2 * sigmoid for the modulations).

Rounding: float64 -> float32 -> bf16 round-to-nearest-even (what v_cvt_pk_bf16_f32 does to an fp32 accumulator), never
float64 -> bf16 directly.  Rounding points (R = rounded to bf16, f32 = kept in fp32, which the replay carries in f64):

  forward
    wf_off   R    offset convolution's gather output (ops._KPConvGather -> ws_kpconv_gather_fwd_bf16 / _fwd_ex, wf bf16)
    offsets  f32  wf_off @ W_off + b_off, bias in the epilogue, out_f32 (ops._MatmulEpilogueBF16.forward, _xbt16)
    W_off, W R    once, when the contraction depth 15 Ci is a multiple of 32 (_bf16_ok -> _bt16, ops.py _MatmulEpilogueBF16);
                  otherwise (Ci = 16, 48) the forward runs the f32 kernel on the f32 MASTER (ops.py: `b.float()`),
                  unrounded, while the backward's dx still uses the rounded weights
    kp, mod  f32  ws_kpconv_deform_prepare
    wf       R    main gather (ws_kpconv_gather_fwd_def, rows_bf16)
    min_d2   f32
    out      R    main contraction, bf16 output
  backward
    dz = dy       already bf16 (main contraction; Co % 4 == 0 through _act_bwd_colsum16, which rounds an f32 dy)
    dwf      R    dz @ R(W)^T (bf16 MFMA, or f32 kernel on widened operands, then rounded)
    dW       f32  wf^T R(dz)
    dx_main  R    ws_kpconv_gather_bwd_x_def / _x_grid_wide (fp32 sum, one rounding)
    d_kp4    f32  ws_kpconv_gather_bwd_geom_def (K6) from the bf16 dwf and x, plus the min_d2 path
    d_off    f32  ws_kpconv_deform_prepare_bwd(d_kp4 + the regulariser's / caller's d deformed_KP)
    dz_off   R    offset contraction, 4K = 60 outputs (% 4 == 0): _act_bwd_colsum16 rounds the f32 d_off; the bias
                  gradient db_off is the f32 column sum of the ROUNDED values (act_bwd_colsum_bf16_kernel re-reads dz)
                  3K = 45 outputs (modulated = False): the f32 _act_bwd_colsum branch, dz_off stays f32 and db_off is
                  its sum; dwf_off is computed from the f32 dz_off, dW_off from R(dz_off) (ops.py: `dz16`)
    dwf_off  R    dz_off @ R(W_off)^T
    dW_off   f32  wf_off^T R(dz_off)
    dx_off   R    rigid gather backward
    dx       R    R(dx_main) + R(dx_off): the autograd accumulation of two bf16 gradients is a bf16 add

``rounding=False`` makes every R the identity: the replay is then the float64 form of the module path under
oracle.kpconv_ref.cpu_reference_mode() (tests/test_oracle_cpu_kpconv.py ties the two together).

Chunked over queries: the [n, H, K, 3] / [n, H, Ci] temporaries of a chunk stay below ~60 MB each at H = 519.
"""
import torch

from oracle.kpconv_ref import kpconv_gather_ref

_ELEMS = 6_000_000          # per-chunk budget of one [n, H, max(3K, Ci)] float64 temporary


def to_bf16(t):
    """float64 -> float32 -> bf16 (RNE) -> float64"""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


class _RoundFwd(torch.autograd.Function):
    """a value the kernel stores in bf16; its gradient passes unchanged (the backward kernels read the stored value)"""

    @staticmethod
    def forward(ctx, t):
        return to_bf16(t)

    @staticmethod
    def backward(ctx, g):
        return g


class _Contraction(torch.autograd.Function):
    """y = x @ w (+ bias): ops._MatmulEpilogueBF16 without residual / activation, with its rounding points"""

    @staticmethod
    def forward(ctx, x, w, bias, out_f32, rounding, trace):
        k, n = w.shape
        wr = to_bf16(w) if rounding else w
        y = x @ (wr if k % 32 == 0 else w)              # _bf16_ok: bf16 MFMA on _bt16(w); else the f32 master
        if bias is not None:
            y = y + bias
        if rounding and not out_f32:
            y = to_bf16(y)
        ctx.save_for_backward(x, wr)
        ctx.cfg = (bias is not None, rounding, trace)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wr = ctx.saved_tensors
        has_bias, rounding, trace = ctx.cfg
        n = wr.shape[1]
        rnd = to_bf16 if rounding else (lambda t: t)
        dz = rnd(dy) if n % 4 == 0 else dy               # _act_bwd_colsum16 (bf16 dz) / _act_bwd_colsum (f32 dz)
        db = dz.sum(0) if has_bias else None
        dx = rnd(dz @ wr.t())
        dz16 = rnd(dz)
        dw = x.t() @ dz16
        if trace is not None:
            trace.setdefault("dz%d" % n, []).append(dz16.detach())
            trace.setdefault("dwf%d" % n, []).append(dx.detach())
        return dx, dw, db, None, None, None


def _chunks(nq, h, width):
    step = max(16, _ELEMS // max(1, h * width))
    return [(a, min(nq, a + step)) for a in range(0, nq, step)]


def _f64(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


def _leaf(t):
    return t.detach().to("cpu", torch.float64).clone().requires_grad_(True)


def replay_rigid(x, q_pts, s_pts, inds, kernel_points, extent, weights, dy, bias=None, out_f32=False, rounding=True,
                 trace=None):
    """a rigid bf16 KPConv (linear influence, sum) -> dict(out, dx, dW, db): the offset convolution of a deformable layer
    when out_f32 and bias are given.  dy: the upstream gradient of out."""
    nq, h = inds.shape
    R = _RoundFwd.apply if rounding else (lambda t: t)   # weights: [K, Ci, Co] or [K Ci, Co]; dW comes back [K Ci, Co]
    xl, wl = _leaf(x), _leaf(weights.reshape(-1, weights.shape[-1]))
    bl = _leaf(bias) if bias is not None else None
    q, s, ii, kp, g = _f64(q_pts), _f64(s_pts), inds.cpu(), _f64(kernel_points), _f64(dy)
    outs = []
    for a, b in _chunks(nq, h, max(3 * kp.shape[0], x.shape[1])):
        wf, _ = kpconv_gather_ref(xl, q[a:b], s, ii[a:b], kp, extent)
        wf = R(wf)
        if trace is not None:
            trace.setdefault("wf_off" if out_f32 else "wf", []).append(wf.detach())
        y = _Contraction.apply(wf.reshape(b - a, -1), wl, bl, out_f32, rounding, trace)
        (y * g[a:b]).sum().backward()
        outs.append(y.detach())
    dx = xl.grad if xl.grad is not None else torch.zeros_like(xl)
    return {"out": torch.cat(outs), "dx": to_bf16(dx) if rounding else dx, "dW": wl.grad,
            "db": bl.grad if bl is not None else None}


def replay_deformable(x, q_pts, s_pts, inds, kernel_points, extent, weights, dy, offset_weights=None, offset_bias=None,
                      offset_kernel_points=None, offsets=None, modulated=True, g_min_d2=None, g_dkp=None, rounding=True,
                      trace=None):
    """one deformable (+ modulated) bf16 KPConv layer and the backward of
        loss = <out, dy> + <min_d2, g_min_d2> + <deformed_KP, g_dkp>
    offsets given (f32 [nq, 3K | 4K]): the geometry is held fixed (no offset convolution; d_off is its gradient);
    otherwise they come from the offset convolution (offset_weights, offset_bias, offset_kernel_points).
    -> dict of float64 CPU tensors: out, wf, offsets, deformed_KP, modulations, min_d2, dx, dx_main, dx_off, dW, d_off,
    dW_off, db_off"""
    nq, h = inds.shape
    K = kernel_points.shape[0]
    R = _RoundFwd.apply if rounding else (lambda t: t)
    rnd = to_bf16 if rounding else (lambda t: t)
    fixed = offsets is not None
    xm, wl = _leaf(x), _leaf(weights.reshape(-1, weights.shape[-1]))
    xo = _leaf(x)
    if not fixed:
        wol, bol = _leaf(offset_weights.reshape(-1, offset_weights.shape[-1])), _leaf(offset_bias)
        okp = _f64(offset_kernel_points if offset_kernel_points is not None else kernel_points)
    q, s, ii, kp = _f64(q_pts), _f64(s_pts), inds.cpu(), _f64(kernel_points)
    g, g1, g2 = _f64(dy), _f64(g_min_d2), _f64(g_dkp)
    off_all = _f64(offsets)
    keep = {k: [] for k in ("out", "wf", "offsets", "deformed_KP", "modulations", "min_d2", "d_off")}
    for a, b in _chunks(nq, h, max(3 * K, x.shape[1])):
        if fixed:
            off = off_all[a:b].clone().requires_grad_(True)
        else:
            wf_off, _ = kpconv_gather_ref(xo, q[a:b], s, ii[a:b], okp, extent)
            wf_off = R(wf_off)
            if trace is not None:
                trace.setdefault("wf_off", []).append(wf_off.detach())
            off = _Contraction.apply(wf_off.reshape(b - a, -1), wol, bol, True, rounding, trace)
            off.retain_grad()
        unscaled = off[:, :3 * K].reshape(-1, K, 3)
        mod = 2 * torch.sigmoid(off[:, 3 * K:]) if modulated else None
        dkp = unscaled * extent + kp
        wf, min_d2 = kpconv_gather_ref(xm, q[a:b], s, ii[a:b], kp, extent, deformed_kp=dkp, modulations=mod)
        wf = R(wf)
        out = _Contraction.apply(wf.reshape(b - a, -1), wl, None, False, rounding, trace)
        loss = (out * g[a:b]).sum()
        if g1 is not None:
            loss = loss + (min_d2 * g1[a:b]).sum()
        if g2 is not None:
            loss = loss + (dkp * g2[a:b]).sum()
        loss.backward()
        for k_, v in (("out", out), ("wf", wf), ("offsets", off), ("deformed_KP", dkp), ("min_d2", min_d2),
                      ("modulations", mod), ("d_off", off.grad)):
            if v is not None:
                keep[k_].append(v.detach())
    res = {k_: (torch.cat(v) if v else None) for k_, v in keep.items()}
    z = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    res["dx_main"] = rnd(z(xm))
    res["dx_off"] = rnd(z(xo))
    res["dx"] = rnd(res["dx_main"] + res["dx_off"]) if not fixed else res["dx_main"]
    res["dW"] = wl.grad
    res["dW_off"] = None if fixed else wol.grad
    res["db_off"] = None if fixed else bol.grad
    return res
