"""GPU: the gradient chain of a deformable + modulated KPConv on bf16 feature rows (BASELINE config 5) against the float64
rounding replay oracle/kpconv_bf16_ref.py, which rounds to bf16 where the HIP path rounds and nowhere else.

Why a replay: the fp32 twin of tests/test_config5_wide_gpu.py sees bf16-rounded INPUTS only.  The GPU also rounds the
offset convolution's wf_off, which moves the offsets by ~1e-2 extents; d w / d kp of the linear influence jumps at the
influence extent (models/blocks.py:337), so against the twin nearly every row of d offset_features holds a flipped
(neighbour, kernel point) pair and no per-row bound is possible.  Against the replay the geometry agrees to fp32, and
what is left is fp32 accumulation order and the rounding ties it decides.

Three stages, so that a failure names its kernel:
  (a) geometry held fixed -- a leaf `off` through ops.deform_prepare -> ops.kpconv_gather_def -> ops.matmul_epilogue:
      ws_kpconv_gather_fwd_def, the bf16 contraction, ws_kpconv_gather_bwd_x_def / _x_grid_wide (rows_bf16 = 1) and K6
      (ws_kpconv_gather_bwd_geom_def), under loss <out, dy> + <min_d2, g1> + <deformed_KP, g2> so that K6's d_min_d2
      input and the prepare backward's d_deformed_kp input are live;
  (b) the offset convolution alone (rigid, _out_f32, _bias) under a fixed f32 upstream gradient: the d_off -> bf16 dz
      rounding, the column-sum bias gradient, dwf_off and the rigid bf16 gather backward;
  (c) the KPConv module, composed, from the same masters.

Tolerances, from the rounding model (u = 2^-9; one bf16 ulp is 2^-7 |r| at the bottom of a binade, 1 -> 1 + 2^-7);
the numbers are in SHARED / COMPOSED below: floors, fractions and fp32 bounds about 4x the largest value measured;
the per-element ulp terms are the model itself (measured ratios up to 0.99 for wf, 0.8 for out, 0.53 for dx):
  * bf16-valued tensors (wf, out, dx): both sides round the same quantity once; they differ only where the fp32 value of
    the GPU and the float64 value of the replay straddle a rounding boundary (a tie, ~1e-4 of the elements), and then by
    one ulp -- or, downstream of a tie, by one ulp of an upstream term times its weight, which under cancellation can
    exceed an ulp of the result.  Held: |a - r| <= 2^-7 |r| + 1e-6 max|r| per element for wf, and
    |a - r| <= 2 x 2^-7 |r| + floor max|r| for out and dx (their own ulp plus what a tie upstream moves them by: one
    upstream ulp), and a cap on the fraction of elements that differ at all.  dx of the composed layer is
    R(R(dx_main) + R(dx_off)): its ulp term is taken of |dx| + |dx_main| + |dx_off|.
  * fp32 tensors (min_d2, deformed_KP, offsets, dW, dW_off, db_off): fp32 re-association of sums of bf16 products and,
    downstream of a tie, one ulp of one term, relative to the tensor's maximum.
  * d offset_features per row (max over the row / max of the tensor) outside the boundary rows, and as one vector.
    A boundary row holds a (neighbour, kernel point) pair within the window of the influence extent, or two neighbours
    within the window of each other's distance to a kernel point (the arg-min that receives d min_d2 switches).  The
    window is 2e-6 extents where the geometry is shared ((a)) and max(2e-6, 2 |kp_gpu - kp_replay|_row / extent) where
    each side runs its own offset convolution ((c)); rows beyond the bound must be boundary rows, at most max(8, 0.5 %).
  * (c) keeps looser bounds than (a) / (b): a tie in wf_off moves the offsets by ~2e-4 of their maximum, wf follows
    continuously and ~2-3 % of the later bf16 roundings flip.
Measured values are written next to the pass / fail with the _report of tests/test_config5_wide_gpu.py (keys chain_*).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
K = 15

# Bounds: about 4x the largest value measured over the cases of this file, tests/test_bf16_gpu.py and the real-width
# cases of tests/test_config5_wide_gpu.py (measured maxima in the comments).  SHARED: stages (a) and (b), the same
# geometry on both sides; COMPOSED: stage (c) and the module tests, each side's own offsets.
SHARED = dict(
    floor_wf=1e-6,        # wf: rounded from the same inputs: one ulp (2^-7 |r|) and no more
    floor=3e-4,           # out, dx: their own ulp plus what a tie upstream moves them by -- up to an ulp of the element
                          # (2 x 2^-7 |r|) or, near zero, one ulp of one input term (3.5e-5 of the max)
    frac=5e-3,            # out differs at 1.8e-3 of its elements (15 Ci inputs per element), dx at 2.3e-4, wf at 1e-4
    geom=1e-6,            # min_d2, deformed_KP (1.7e-7)
    dW=1.5e-3,            # dW (4.1e-4), dW_off (6.0e-4) and offsets (4.2e-4): one tie-moved term in an fp32 sum
    db_off=1e-6,          # the column sum of the rounded d offset_features (1.6e-7)
    row=7e-4, row_l2=2e-5)  # d offset_features per row (1.7e-4) and as one vector (5.1e-6)
COMPOSED = dict(
    floor=1.5e-3,         # the offsets differ by ~2e-4 (a wf_off tie moves them): wf moves continuously, out / dx by 3.9e-4
    frac=0.12,            # ... and ~2-3 % of the bf16 roundings flip (3.1 %)
    geom=1e-3,            # min_d2, deformed_KP (2.5e-4)
    dW=3e-3,              # dW, dW_off, db_off, offsets (8.8e-4) where no row flipped; with a flipped row dW_off / db_off
    dW_l2=8e-3,           #   are held as one vector (2.0e-3)
    row=2e-3, row_l2=2e-4)  # d offset_features outside the windows (7.1e-4 per row, 4.1e-5 as one vector)


def _report(key, values):
    from test_config5_wide_gpu import _report as report
    report("chain_" + key, values)


def _np(t):
    return t.detach().double().cpu()


def bf_err(a, r, floor, scale=None, ulps=2):
    """(max of |a - r| / (ulps 2^-7 scale + floor max|r|), fraction of elements that differ beyond 1e-6 max|r|);
    scale defaults to |r| (2^-7 |r| >= one ulp of the element)"""
    if r.numel() == 0:
        return 0.0, 0.0
    a, r = _np(a).reshape(r.shape[0], -1), r.detach().double().reshape(r.shape[0], -1)
    m = float(r.abs().max().clamp_min(1e-30))
    d = (a - r).abs()
    sc = r.abs() if scale is None else scale.reshape(r.shape)
    return float((d / (ulps * 2.0 ** -7 * sc + floor * m)).max()), float((d > 1e-6 * m).double().mean())


def f32_err(a, r):
    a, r = _np(a).reshape(r.shape), r.detach().double()
    return float((a - r).abs().max() / r.abs().max().clamp_min(1e-30))


def boundary_rows(q_pts, s_pts, inds, dkp, extent, window):
    """rows where the gradient of the geometry may jump when the kernel points move by `window` extents (per row):
    a (neighbour, kernel point) pair within `window` of the influence extent (d w / d kp jumps there, models/blocks.py:337),
    or two neighbours whose distances to a kernel point are that close (the arg-min that receives d min_d2 switches)"""
    s_pad = torch.cat((s_pts.cpu().double(), torch.zeros(1, 3, dtype=torch.float64) + 1e6), 0)
    qc, ic = q_pts.cpu().double(), inds.cpu()
    near = torch.zeros(qc.shape[0], dtype=torch.bool)
    for a in range(0, qc.shape[0], 256):
        nb = s_pad[ic[a:a + 256]] - qc[a:a + 256].unsqueeze(1)
        d = torch.sqrt(((nb.unsqueeze(2) - dkp[a:a + 256].unsqueeze(1)) ** 2).sum(3))       # [n, H, K]
        w = window[a:a + 256, None, None]
        edge = ((d / extent - 1).abs() < w).flatten(1).any(1)
        two = torch.topk(d, 2, dim=1, largest=False).values if d.shape[1] > 1 else torch.cat((d, d + 1e9), 1)
        tie = ((two[:, 1] - two[:, 0]) / extent < 2 * w[:, :, 0]).any(1)
        near[a:a + 256] = edge | tie
    return near


def row_errs(got, want):
    """per-row max error / tensor max, and the L2 relative error"""
    g, w = _np(got), want.detach().double()
    scale = float(w.abs().max().clamp_min(1e-30))
    return (g - w).abs().amax(dim=1) / scale, g, w


def check_rows(errs, name, got, want, near, row):
    """rows of a geometry gradient beyond `row` (-> bool [nrows]); their maximum and L2 outside the boundary window"""
    re, g, w = row_errs(got, want)
    bad = re > row
    clean = ~near
    errs[name + "_rows"] = float(re[clean].max()) if bool(clean.any()) else 0.0
    errs[name + "_l2"] = float((g[clean] - w[clean]).norm() / w[clean].norm().clamp_min(1e-30))
    errs[name + "_flipped"] = int(bad.sum())
    errs["boundary_rows"] = int(near.sum())
    return bad


def _inputs(nq, ns, ci, co, modulated, seed, gpu):
    torch.manual_seed(seed)
    od = (4 if modulated else 3) * K
    off = torch.randn(nq, od, device=gpu) * 0.15                 # ~0.15 extents (what _layer_pair's offsets reach)
    if modulated:
        off[:, 3 * K:] = torch.randn(nq, K, device=gpu)
    W = torch.randn(K * ci, co, device=gpu) / (K * ci) ** 0.5
    x = torch.randn(ns, ci, device=gpu).to(BF)
    dy = torch.randn(nq, co, device=gpu).to(BF)
    return off, W, x, dy


def stage_fixed(gpu, q, s, inds, kp, extent, ci, co, modulated, rows_sorted, seed, grid_expected=None):
    """(a): the geometry held fixed; -> errors, d_off rows flagged bad"""
    from oracle import kpconv_bf16_ref
    from weasal_amd import ops
    nq, ns = q.shape[0], s.shape[0]
    off, W, x, dy = _inputs(nq, ns, ci, co, modulated, seed, gpu)
    if grid_expected is not None:
        assert (ops._grid_for(inds) is not None) == grid_expected, "backward path of dx"

    def run(g1, g2):
        offg, xg, Wg = off.clone().requires_grad_(True), x.clone().requires_grad_(True), W.clone().requires_grad_(True)
        kp4, dkp, _, rmax = ops.deform_prepare(offg, kp, extent, modulated)
        wf, min_d2 = ops.kpconv_gather_def(xg, kp4, q, s, inds, extent, kp_rmax=rmax, rows_sorted=rows_sorted)
        out = ops.matmul_epilogue(wf.reshape(nq, -1), Wg)
        assert wf.dtype == BF and out.dtype == BF and min_d2.dtype == torch.float32
        outs, grads = [out], [dy]
        if g1 is not None:
            outs += [min_d2, dkp]
            grads += [g1, g2]
        torch.autograd.backward(outs, grads)
        return dict(wf=wf, out=out, min_d2=min_d2, dkp=dkp, dx=xg.grad, dW=Wg.grad, d_off=offg.grad)

    # g1 / g2 sized so that each of the three paths into d_off carries a comparable share of it
    s_ = float(run(None, None)["d_off"][:, :3 * K].abs().max())
    g1 = torch.randn(nq, K, device=gpu) * (0.3 * s_ / (2 * extent ** 2))
    g2 = torch.randn(nq, K, 3, device=gpu) * (0.3 * s_ / extent)
    got = run(g1, g2)
    torch.cuda.synchronize()
    rep = kpconv_bf16_ref.replay_deformable(x, q, s, inds, kp, extent, W, dy, offsets=off, modulated=modulated,
                                            g_min_d2=g1, g_dkp=g2)
    errs = {}
    for k_ in ("wf", "out", "dx"):
        rk = {"dx": "dx_main"}.get(k_, k_)
        errs[k_], errs[k_ + "_frac"] = bf_err(got[k_], rep[rk], SHARED["floor_wf" if k_ == "wf" else "floor"],
                                              ulps=1 if k_ == "wf" else 2)
    errs["min_d2"] = f32_err(got["min_d2"], rep["min_d2"])
    errs["deformed_KP"] = f32_err(got["dkp"], rep["deformed_KP"])
    errs["dW"] = f32_err(got["dW"], rep["dW"])
    near = boundary_rows(q, s, inds, rep["deformed_KP"], extent, torch.full((nq,), 2e-6, dtype=torch.float64))
    bad = check_rows(errs, "d_off", got["d_off"], rep["d_off"], near, SHARED["row"])
    return errs, bad, near


def stage_offset_conv(gpu, q, s, inds, ci, extent, radius, modulated, rows_sorted, seed):
    """(b): the offset convolution alone: rigid bf16 KPConv, f32 output, bias in the epilogue"""
    from oracle import kpconv_bf16_ref
    conv = _module(gpu, ci, 32, extent, radius, modulated)
    torch.manual_seed(seed)
    x = torch.randn(s.shape[0], ci, device=gpu).to(BF)
    d_up = torch.randn(q.shape[0], conv.offset_dim, device=gpu)
    xg = x.clone().requires_grad_(True)
    off = conv.offset_conv(q, s, inds, xg, _bias=conv.offset_bias, _out_f32=True, _rows_sorted=rows_sorted)
    assert off.dtype == torch.float32
    off.backward(d_up)
    torch.cuda.synchronize()
    rep = kpconv_bf16_ref.replay_rigid(x, q, s, inds, conv.offset_conv.kernel_points, extent, conv.offset_conv.weights, d_up,
                                       bias=conv.offset_bias, out_f32=True)
    errs = {"offsets": f32_err(off, rep["out"]), "dW_off": f32_err(conv.offset_conv.weights.grad.reshape(-1, conv.offset_dim), rep["dW"]),
            "db_off": f32_err(conv.offset_bias.grad, rep["db"])}
    errs["dx"], errs["dx_frac"] = bf_err(xg.grad, rep["dx"], SHARED["floor"])
    return errs


def _module(gpu, ci, co, extent, radius, modulated):
    from weasal_amd.blocks import KPConv
    np.random.seed(1)
    torch.manual_seed(1)
    conv = KPConv(K, 3, ci, co, extent, radius, deformable=True, modulated=modulated)
    with torch.no_grad():                   # offsets of a useful size (the zero-mean init gives ~0.01 extents)
        conv.offset_conv.weights.mul_(4.0 * (32.0 / ci) ** 0.5)
        conv.offset_bias.normal_(0.0, 0.05)
    return conv.to(gpu)


def replay_module(conv, x, q, s, inds, dy, g1=None, g2=None):
    from oracle import kpconv_bf16_ref
    return kpconv_bf16_ref.replay_deformable(x, q, s, inds, conv.kernel_points, conv.KP_extent, conv.weights, dy,
                                             offset_weights=conv.offset_conv.weights, offset_bias=conv.offset_bias,
                                             offset_kernel_points=conv.offset_conv.kernel_points, modulated=conv.modulated,
                                             g_min_d2=g1, g_dkp=g2)


def compare_module(conv, rep, out, x_grad, d_off, q, s, inds, errs, clean_sets=True):
    """(c) / the tightened module tests: the module's results against the replay; -> (bad rows, clean_q, clean_s)"""
    nq = q.shape[0]
    extent = conv.KP_extent
    dkp_g = _np(conv.deformed_KP)
    moved = (dkp_g - rep["deformed_KP"]).norm(dim=2).amax(dim=1) / extent
    errs["kp_moved"] = float(moved.max())
    window = torch.clamp(2 * moved, min=2e-6)
    near = boundary_rows(q, s, inds, rep["deformed_KP"], extent, window)
    bad = check_rows(errs, "d_off", d_off, rep["d_off"], near, COMPOSED["row"])
    errs["offsets"] = f32_err(conv.offset_features, rep["offsets"])
    errs["deformed_KP"] = f32_err(conv.deformed_KP, rep["deformed_KP"])
    errs["min_d2"] = f32_err(conv.min_d2, rep["min_d2"])
    errs["out"], errs["out_frac"] = bf_err(out, rep["out"], COMPOSED["floor"])
    errs["dW"] = f32_err(conv.weights.grad.reshape(-1, conv.out_channels), rep["dW"])
    clean_q = ~bad
    touched = torch.zeros(s.shape[0] + 1, dtype=torch.bool)
    touched[inds.cpu()[bad].flatten()] = True
    clean_s = ~touched[:-1]
    # dx = R(R(dx_main) + R(dx_off)): a tie in either term moves the sum by an ulp of that term
    sc = rep["dx"].abs() + rep["dx_main"].abs() + rep["dx_off"].abs()
    errs["dx"], errs["dx_frac"] = bf_err(_np(x_grad)[clean_s], rep["dx"][clean_s], COMPOSED["floor"], sc[clean_s])
    od = conv.offset_dim
    errs["dW_off"] = f32_err(conv.offset_conv.weights.grad.reshape(-1, od), rep["dW_off"])
    errs["db_off"] = f32_err(conv.offset_bias.grad, rep["db_off"])
    l2 = lambda a, r: float((_np(a).reshape(r.shape) - r).norm() / r.norm().clamp_min(1e-30))
    errs["dW_off_l2"] = l2(conv.offset_conv.weights.grad, rep["dW_off"])
    errs["db_off_l2"] = l2(conv.offset_bias.grad, rep["db_off"])
    return bad, near, clean_q, clean_s


def assert_chain(errs, bad, near, nrows, key, b):
    """the bounds `b` (SHARED or COMPOSED) on whatever keys a stage measured"""
    for k_ in ("wf", "out", "dx"):
        if k_ in errs:
            assert errs[k_] <= 1.0 and errs[k_ + "_frac"] <= b["frac"], (key, k_, errs)
    for k_ in ("min_d2", "deformed_KP"):
        if k_ in errs:
            assert errs[k_] <= b["geom"], (key, k_, errs)
    flipped = errs.get("d_off_flipped", 0) > 0
    for k_ in ("offsets", "dW", "dW_off", "db_off"):
        if k_ in errs:
            if flipped and k_ in ("dW_off", "db_off"):
                # sums over all rows: the flipped rows' (legitimately different) terms are in them
                assert errs[k_ + "_l2"] <= b["dW_l2"], (key, k_, errs)
            else:
                assert errs[k_] <= b.get(k_, b["dW"]), (key, k_, errs)
    if bad is not None:
        assert errs["d_off_rows"] <= b["row"] and errs["d_off_l2"] <= b["row_l2"], (key, errs)
        assert int((bad & ~near).sum()) == 0, (key, "rows of d offset_features beyond the bound outside the boundary window", errs)
        assert int(bad.sum()) <= max(8, nrows // 200), (key, errs)


def stage_module(gpu, q, s, inds, ci, co, extent, radius, modulated, rows_sorted, seed):
    """(c): the KPConv module against the replay from the same masters"""
    conv = _module(gpu, ci, co, extent, radius, modulated)
    torch.manual_seed(seed)
    nq = q.shape[0]
    x = torch.randn(s.shape[0], ci, device=gpu).to(BF)
    dy = torch.randn(nq, co, device=gpu).to(BF)
    got = {}

    def run(g1, g2):
        conv.zero_grad()
        xg = x.clone().requires_grad_(True)
        out = conv(q, s, inds, xg, _rows_sorted=rows_sorted)
        assert out.dtype == BF
        conv.offset_features.register_hook(lambda g_: got.__setitem__("d_off", g_.detach()))
        if g1 is None:
            out.backward(dy)
        else:
            torch.autograd.backward([out, conv.min_d2, conv.deformed_KP], [dy, g1, g2])
        return out, xg

    run(None, None)
    s_ = float(got["d_off"][:, :3 * K].abs().max())              # as in stage_fixed
    g1 = torch.randn(nq, K, device=gpu) * (0.3 * s_ / (2 * extent ** 2))
    g2 = torch.randn(nq, K, 3, device=gpu) * (0.3 * s_ / extent)
    out, xg = run(g1, g2)
    torch.cuda.synchronize()
    rep = replay_module(conv, x, q, s, inds, dy, g1, g2)
    errs = {}
    bad, near, _, _ = compare_module(conv, rep, out, xg.grad, got["d_off"], q, s, inds, errs)
    return errs, bad, near


# ---------------------------------------------------------------------------------------------------------------------
# real widths: the config-5 cases of tests/test_config5_wide_gpu.py
# ---------------------------------------------------------------------------------------------------------------------
def _wide_layer(gpu, kind, lvl):
    from test_config5_wide_gpu import LIMITS, _small_dense_batch
    cfg, batch = _small_dense_batch(gpu)
    batch.activate()
    r = cfg.first_subsampling_dl * cfg.conv_radius * 2 ** lvl
    extent = r * cfg.KP_extent / cfg.conv_radius
    if kind == "self":
        q = s = batch.points[lvl]
        inds = batch.neighbors[lvl]
    else:
        q, s, inds = batch.points[lvl + 1], batch.points[lvl], batch.pools[lvl]
    assert inds.shape[1] == min(LIMITS[lvl], inds.shape[1]) and (lvl > 1 or inds.shape[1] == LIMITS[lvl])
    return q, s, inds, r, extent


WIDE = [("self", 0, 32), ("strided", 0, 32), ("self", 1, 64), ("strided", 1, 64), ("self", 2, 128)]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("kind,lvl,ci", WIDE)
def test_bf16_chain_real_width(gpu, kind, lvl, ci):
    from weasal_amd import ops
    from weasal_amd.kernel_points import load_kernels
    q, s, inds, r, extent = _wide_layer(gpu, kind, lvl)
    rows_sorted = ops.rows_cutoff_pays(inds, r)
    np.random.seed(3)
    kp = torch.from_numpy(load_kernels(r, K, dimension=3, fixed="center").astype(np.float32)).to(gpu)
    # self-query layers take the table-free grid backward (ws_kpconv_gather_bwd_x_grid_wide), strided ones (queries !=
    # supports) the transposed table (ws_kpconv_gather_bwd_x_def)
    grid = True if (kind == "self" and ops.GRID_BACKWARD and lvl < 2) else None
    assert (kind == "self") == (q.data_ptr() == s.data_ptr())
    key = "%s_l%d_c%d" % (kind, lvl, ci)
    ea, bad_a, near_a = stage_fixed(gpu, q, s, inds, kp, extent, ci, ci, True, rows_sorted, 11 + lvl, grid_expected=grid)
    _report(key + "_a", ea)
    assert_chain(ea, bad_a, near_a, q.shape[0], key + "_a", SHARED)
    eb = stage_offset_conv(gpu, q, s, inds, ci, extent, r, True, rows_sorted, 21 + lvl)
    _report(key + "_b", eb)
    assert_chain(eb, None, None, q.shape[0], key + "_b", SHARED)
    ec, bad_c, near_c = stage_module(gpu, q, s, inds, ci, ci, extent, r, True, None, 31 + lvl)
    _report(key + "_c", ec)
    assert_chain(ec, bad_c, near_c, q.shape[0], key + "_c", COMPOSED)


# ---------------------------------------------------------------------------------------------------------------------
# small shapes: the fallbacks of the contraction and the switches of the gather kernels
# ---------------------------------------------------------------------------------------------------------------------
def _small_geometry(gpu, n, radius, seed, strided):
    """uniform points, rows from the radius search (sorted by distance) at twice the convolution radius (the deformable
    search radius), so that the sorted-row cutoff has columns to skip"""
    from weasal_amd import ops
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-3, 3, size=(n, 3)).astype(np.float32)
    lens = np.array([n // 2, n - n // 2], np.int32)
    P = torch.from_numpy(pts).to(gpu)
    if not strided:
        return P, P, ops.radius_neighbors(P, P, lens, lens, 2 * radius, dtype=torch.int64)
    Q = P[::4].contiguous()
    ql = np.array([len(range(0, int(lens[0]), 4)), 0], np.int32)
    ql[1] = Q.shape[0] - ql[0]
    return Q, P, ops.radius_neighbors(Q, P, ql, lens, 2 * radius, dtype=torch.int64)


SMALL = [  # ci, co, modulated, rows_sorted, strided
    pytest.param(16, 32, True, True, False, id="ci16-f32fallback-sorted"),
    pytest.param(48, 32, True, False, True, id="ci48-f32fallback-unsorted-strided"),
    pytest.param(32, 32, False, True, False, id="ci32-unmodulated-sorted"),
    pytest.param(32, 30, True, False, False, id="ci32-co30-unsorted"),
    pytest.param(64, 64, True, True, True, id="ci64-sorted-strided"),
]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("ci,co,modulated,rows_sorted,strided", SMALL)
def test_bf16_chain_small(gpu, ci, co, modulated, rows_sorted, strided):
    from weasal_amd import ops
    from weasal_amd.kernel_points import load_kernels
    ops.clear_batch_hints()
    radius = 0.6
    extent = 0.4 * radius
    q, s, inds = _small_geometry(gpu, 5000, radius, ci + co, strided)
    assert ops._grid_for(inds) is None                       # no batch hints: the transposed-table backward
    np.random.seed(3)
    kp = torch.from_numpy(load_kernels(radius, K, dimension=3, fixed="center").astype(np.float32)).to(gpu)
    key = "small_c%d_o%d_m%d_s%d_t%d" % (ci, co, modulated, rows_sorted, strided)
    ea, bad_a, near_a = stage_fixed(gpu, q, s, inds, kp, extent, ci, co, modulated, rows_sorted, 41)
    _report(key + "_a", ea)
    assert_chain(ea, bad_a, near_a, q.shape[0], key + "_a", SHARED)
    eb = stage_offset_conv(gpu, q, s, inds, ci, extent, radius, modulated, rows_sorted, 42)
    _report(key + "_b", eb)
    assert_chain(eb, None, None, q.shape[0], key + "_b", SHARED)
    ec, bad_c, near_c = stage_module(gpu, q, s, inds, ci, co, extent, radius, modulated, rows_sorted, 43)
    _report(key + "_c", ec)
    assert_chain(ec, bad_c, near_c, q.shape[0], key + "_c", COMPOSED)
