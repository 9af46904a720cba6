"""The KPConv gather kernels at 9 and 13 kernel points, every launch branch held to a float64 reference per element.

The harness of tests/test_kpconv_branches_gpu.py (K = 15) at K in {9, 13}: the same lattice clouds, EXTENT / RADIUS constants,
reference (oracle.kpconv_branch_ref: ref_forward / ref_backward in float64) and per-element bounds (fwd_bound, dx_bound,
geom_bounds, min_d2_bound -- the error model, never a fraction of the tensor's maximum), with kernel points from
lattice_kernel(rng, K, reach).  `BRANCHES` states, row by row, what a public entry launches for the new sizes; before a launch
the library's reporter (ws_kpconv_gather_variant_k) has to name the row with the size in its text; every row's setup asserts
the extent margin and, for `closest`, that no neighbour is equidistant from two kernel points.  f32 rows only: bf16 rows,
MODE 2 and the fused layer stay K = 15 (refusals: tests/test_kpconv_ksize_cpu.py).

  K3 matrix core   one 16-row A tile, rows >= K masked: every NT, the SPLIT_NT / csplit narrowing below SPLIT_ROWS, masked NT = 1
                   rows (ci = 100), MODE 1 through gaussian / constant / closest, DEF (+ modulations) with min_d2, CUT
  K3 VALU          ci = 4 (G = 1, float4) and ci = 3 (G = 4, 4-byte pieces); K = 13 walks the kernel points one per trip (KU)
  K4               every G, MODE 0 / 1, the packed form (four supports per wave) bit-identical to the single-support form
  K6               the VALU geometry backward, float4 and scalar rows
  K4G              slab form bit-identical to the table form in index order, within twice the summation bound in walk order;
                   the wide (queue) form, MODE 0
  deform.hip       ws_kpconv_deform_prepare / _bwd and ws_p2p_regularizer_fwd / _bwd against oracle/deform_ref.py
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import test_kpconv_branches_gpu as GB
from oracle import deform_ref as D
from oracle import kpconv_branch_ref as R

pytestmark = pytest.mark.gpu

SIZES = (9, 13)
EXTENT, RADIUS, KP_REACH = GB.EXTENT, GB.RADIUS, GB.KP_REACH
MF, VF, K4, K6 = GB.MF, GB.VF, GB.K4, GB.K6
PACKED = "kpconv_gather_bwd_x_packed_kernel"


def _mf(k, nt, mode, deff, cut=False):
    return "K=%d, " % k + GB._mf(nt, mode, deff, "float", cut)


def _vf(k, g, mode, deff, vec, pw):
    return GB._vf(g, mode, deff, vec, pw, "float").replace("K=15", "K=%d" % k)


def _k4(k, g, mode, vec):
    return (K4, "K=%d, G=%d, MODE=%d, VEC=%s, T=float" % (k, g, mode, "true" if vec else "false"))


def _k6(k, vec):
    return (K6, "K=%d, T=float (vec4=%d)" % (k, 1 if vec else 0))


def _b(id, k, kernel, targs, ci, nq, **kw):
    entry = "ws_kpconv_gather_fwd_ex" if kw.get("rows_sorted") else "ws_kpconv_gather_fwd"
    row = GB._b("k%d_%s" % (k, id), entry, kernel, targs, ci, nq, **kw)
    row["k"] = k
    return row


BRANCHES = []
for _k in SIZES:
    BRANCHES += [
        # ---- K3 on the matrix core, every NT
        _b("k3_nt1", _k, MF, _mf(_k, 1, 0, False), 16, 600),
        _b("k3_nt2", _k, MF, _mf(_k, 2, 0, False), 32, 600, bwd=_k4(_k, 8, 0, True)),
        _b("k3_nt4", _k, MF, _mf(_k, 4, 0, False), 64, 600),
        _b("k3_nt8", _k, MF, _mf(_k, 8, 0, False), 128, 4096),
        _b("k3_nt16", _k, MF, _mf(_k, 16, 0, False), 256, 4096),
        # ---- one query below SPLIT_ROWS: SPLIT_NT narrowing + csplit items
        _b("k3_split128", _k, MF, _mf(_k, 4, 0, False), 128, 4095, csplit=2),
        _b("k3_split256", _k, MF, _mf(_k, 4, 0, False), 256, 4095, csplit=4),
        # ---- ci % nt != 0: masked NT = 1 rows, partial last block (100 = 6 x 16 + 4)
        _b("k3_ci100_split", _k, MF, _mf(_k, 1, 0, False), 100, 600, csplit=7),
        _b("k3_ci100_loop", _k, MF, _mf(_k, 1, 0, False), 100, 4096),
        # ---- MODE 1 through each influence / aggregation
        _b("k3_gauss", _k, MF, _mf(_k, 2, 1, False), 32, 600, influence="gaussian", bwd=_k4(_k, 8, 1, True)),
        _b("k3_const", _k, MF, _mf(_k, 4, 1, False), 64, 600, influence="constant"),
        _b("k3_closest", _k, MF, _mf(_k, 8, 1, False), 128, 64, aggregation="closest", bwd=_k4(_k, 16, 1, True)),
        # ---- deformable (the generic entries: what a deformable layer of these sizes runs): MODE 1 + DEF, min_d2, K4 MODE 1, K6
        _b("k3_def", _k, MF, _mf(_k, 2, 1, True), 32, 600, deform="def", bwd=_k4(_k, 8, 1, True), geom=_k6(_k, True)),
        _b("k3_defmod", _k, MF, _mf(_k, 4, 1, True), 64, 600, deform="defmod", bwd=_k4(_k, 16, 1, True), geom=_k6(_k, True)),
        _b("k3_defmod_ci20", _k, MF, _mf(_k, 2, 1, True), 20, 400, deform="defmod", bwd=_k4(_k, 8, 1, True), geom=_k6(_k, True)),
        _b("k3_defmod_ci30", _k, MF, _mf(_k, 2, 1, True), 30, 400, deform="defmod", bwd=_k4(_k, 8, 1, False), geom=_k6(_k, False)),
        _b("k3_def_closest", _k, MF, _mf(_k, 1, 1, True), 16, 64, aggregation="closest", deform="def", bwd=_k4(_k, 4, 1, True),
           geom=_k6(_k, True)),
    ]
    # ---- rows sorted by distance (CUT) on rows of the radius search: every NT
    BRANCHES += [_b("k3_cut_nt%d" % _nt, _k, MF, _mf(_k, _nt, 0, False, cut=True), _ci, 600, rows_sorted=True, rows="search")
                 for _nt, _ci in ((1, 16), (2, 32), (4, 64), (8, 128), (16, 256))]
    BRANCHES += [
        # ---- VALU form, ci <= 4
        _b("valu_ci4", _k, VF, _vf(_k, 1, 0, False, True, 4), 4, 600, bwd=_k4(_k, 1, 0, True)),
        _b("valu_ci3", _k, VF, _vf(_k, 4, 0, False, False, 1), 3, 600, bwd=_k4(_k, 1, 0, False)),
        _b("valu_ci4_gauss", _k, VF, _vf(_k, 1, 1, False, True, 4), 4, 600, influence="gaussian", bwd=_k4(_k, 1, 1, True),
           note="K live kernel points per neighbour: the pool overflows, 16-lane sub-chunks"),
        _b("valu_ci3_def", _k, VF, _vf(_k, 4, 1, True, False, 1), 3, 600, deform="defmod", bwd=_k4(_k, 1, 1, False), geom=_k6(_k, False)),
        _b("valu_ci4_cut", _k, VF, _vf(_k, 1, 0, False, True, 4), 4, 600, rows_sorted=True, rows="search"),
        _b("valu_ci3_h129", _k, VF, _vf(_k, 4, 0, False, False, 1), 3, 300, h=129, queries="dense", bwd=_k4(_k, 1, 0, False),
           note="two column chunks in one pool"),
    ]
    # ---- K4 through the transposed table: every G, fast / generic, on rows where one support has several hundred incoming pairs
    for _ci, _g in ((8, 2), (16, 4), (32, 8), (64, 16), (6, 2)):
        _vec = _ci % 4 == 0
        for _mode, _inf in ((0, "linear"), (1, "gaussian")):
            _nt = 1 if _ci <= 16 else 2 if _ci <= 32 else 4
            _nt = _nt if _ci % _nt == 0 else 1
            _cs = -(-_ci // (16 * _nt)) if (_mode == 0 and _ci > 16 * _nt) else 1
            BRANCHES.append(_b("k4_g%d_%s_ci%d" % (_g, "fast" if _mode == 0 else "generic", _ci), _k, MF, _mf(_k, _nt, _mode, False), _ci,
                               400, h=40, influence=_inf, queries="hub", csplit=_cs, bwd=_k4(_k, _g, _mode, _vec)))


# `closest` rows: 64 queries (16 workgroups) and a seed, found on the CPU, under which no neighbour is equidistant from two kernel
# points -- on these lattices about one pair in 300 is, so larger tie-free clouds are out of a seed search's reach.  (With ties
# the first kernel point wins in the kernels and in the reference alike: the K = 15 table has rows for that.)
SEED_SALT = {"k9_k3_closest": 11, "k9_k3_def_closest": 35, "k13_k3_closest": 6, "k13_k3_def_closest": 56}


def supports_of(row):
    return {"self": row["nq"], "distinct": row["nq"] + 37, "hub": 2001, "dense": 2400}[row["queries"]]


# ------------------------------------------------------------------------------------------------------------------
# the library's own statement of a launch, for k kernel points
# ------------------------------------------------------------------------------------------------------------------
def report(op, k, nq, ns, ci, rows_a, rows_b, deformed=False, modulated=False, influence="linear", aggregation="sum",
           rows_sorted=False, ordered=False):
    from weasal_amd import _lib, ops
    buf = C.create_string_buffer(256)
    _lib.check(_lib.lib().ws_kpconv_gather_variant_k(GB.GATHER_OPS[op], nq, ns, ci, rows_a, rows_b, int(deformed), int(modulated),
                                                     ops.INFLUENCE[influence], ops.AGGREGATION[aggregation], 0, int(rows_sorted),
                                                     int(ordered), k, buf, 256))
    return GB.parse_launch(buf.value.decode())


def check_row_plan(row, ptr, nq, ns):
    """the reporter names what the row says it launches, the size included; -> the number of launches checked"""
    kw = dict(deformed=row["deform"] is not None, modulated=row["deform"] == "defmod", influence=row["influence"],
              aggregation=row["aggregation"])
    kernel, args, keys = report("fwd", row["k"], nq, ns, row["ci"], ptr("x"), ptr("wf"), rows_sorted=row["rows_sorted"], **kw)
    want = GB.table_launch(row["kernel"], row["targs"])
    assert (kernel, args) == want[:2] and args["K"] == str(row["k"]) and keys["csplit"] == row["csplit"], (row["id"], kernel, args, keys)
    checked = 1
    for key, op, a, b in (("bwd", "bwd_x", "dwf", "dx"), ("geom", "bwd_geom", "x", "dwf")):
        if row[key]:
            kernel, args, keys = report(op, row["k"], nq, ns, row["ci"], ptr(a), ptr(b), **kw)
            want = GB.table_launch(*row[key])
            assert (kernel, args) == want[:2] and all(keys[n] == v for n, v in want[2].items()), (row["id"], key, kernel, args, keys)
            checked += 1
    return checked


# ------------------------------------------------------------------------------------------------------------------
# inputs (GB._setup with K kernel points)
# ------------------------------------------------------------------------------------------------------------------
def _setup(row, gpu):
    k = row["k"]
    rng = np.random.default_rng(zlib.crc32(row["id"].encode()) + SEED_SALT.get(row["id"], 0))
    nq, ci = row["nq"], row["ci"]
    kp = R.lattice_kernel(rng, k, KP_REACH)
    if row["queries"] == "hub":
        q = R.lattice_cloud(rng, nq, 0.4)
        s = np.concatenate([R.lattice_cloud(rng, 2000, 1.5), np.zeros((1, 3), np.float32)])   # the hub is the last support
        inds = R.brute_rows(q, s[:-1], RADIUS, row["h"] - 1)
        inds[inds == s.shape[0] - 1] = s.shape[0]
        inds = np.concatenate([np.full((nq, 1), s.shape[0] - 1, np.int64), inds], 1)
    elif row["queries"] == "dense":
        s = R.lattice_cloud(rng, 2400, 1.25)
        q = R.lattice_cloud(rng, nq, 0.45)
        inds = R.brute_rows(q, s, RADIUS, row["h"])
        inds[::7] = s.shape[0]                                   # rows that are all shadow
    else:
        half = GB._half_for(nq, 90 if row["rows"] == "search" else 24)
        s = R.lattice_cloud(rng, nq, half)
        q = s
        if row["rows"] == "search":
            from weasal_amd import ops
            S = torch.from_numpy(s).to(gpu)
            inds = ops.radius_neighbors(S, S, [len(s)], [len(s)], RADIUS, dtype=torch.int64).cpu().numpy()
        else:
            inds = R.brute_rows(q, s, RADIUS, 40)
            inds[::11, 20:] = s.shape[0]                          # shorter rows
    deformed = mod = None
    if row["deform"]:
        deformed = R.lattice_deformed(rng, kp, nq, 0.05)
        if row["deform"] == "defmod":
            mod = rng.uniform(0.25, 1.0, size=(nq, k)).astype(np.float32)
    assert R.extent_margin(q, s, inds, kp, EXTENT, deformed) > 1e-6
    if row["aggregation"] == "closest":
        assert R.closest_tie_count(q, s, inds, kp, deformed) == 0, "closest: a tie between kernel points (choose another seed)"
    x = rng.standard_normal((s.shape[0], ci)).astype(np.float32)
    return dict(q=q, s=s, inds=inds, kp=kp, deformed=deformed, mod=mod, x=x)


def _run(row, d, gpu, dwf=None, dmin=None):
    from weasal_amd import ops
    k = row["k"]
    Q = torch.from_numpy(d["q"]).to(gpu)
    S = Q if row["queries"] == "self" else torch.from_numpy(d["s"]).to(gpu)
    inds = torch.from_numpy(d["inds"]).to(gpu)
    X = torch.from_numpy(d["x"]).to(gpu)
    bufs = dict(x=X, wf=torch.empty((Q.shape[0], k, row["ci"]), device=gpu), dx=torch.empty_like(X))
    if dwf is not None:
        bufs["dwf"] = torch.from_numpy(dwf).to(gpu)
    check_row_plan(row, lambda name: bufs[name].data_ptr(), Q.shape[0], S.shape[0])
    if dwf is not None:
        X = X.detach().requires_grad_(True)
    kw = {}
    if d["deformed"] is not None:
        kw["deformed_kp"] = torch.from_numpy(d["deformed"]).to(gpu).requires_grad_(dwf is not None)
        kw["want_min_d2"] = True
        if d["mod"] is not None:
            kw["modulations"] = torch.from_numpy(d["mod"]).to(gpu).requires_grad_(dwf is not None)
    wf, mn = ops.kpconv_gather(X, Q, S, inds, torch.from_numpy(d["kp"]).to(gpu), EXTENT, row["influence"], row["aggregation"],
                               rows_sorted=row["rows_sorted"], **kw)
    assert tuple(wf.shape) == (Q.shape[0], k, row["ci"])
    out = dict(wf=wf.detach().cpu().numpy(), min_d2=mn.detach().cpu().numpy() if mn is not None else None)
    if dwf is not None:
        G = torch.from_numpy(dwf).to(gpu)
        if mn is not None:
            torch.autograd.backward([wf, mn], [G, torch.from_numpy(dmin).to(gpu)])
        else:
            wf.backward(G)
        out["dx"] = X.grad.cpu().numpy()
        if "deformed_kp" in kw:
            out["d_dkp"] = kw["deformed_kp"].grad.cpu().numpy()
        if "modulations" in kw:
            out["d_mod"] = kw["modulations"].grad.cpu().numpy()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("row", BRANCHES, ids=[r["id"] for r in BRANCHES])
def test_ksize_branch_vs_float64(row, gpu):
    from weasal_amd import ops
    ops.clear_batch_hints()
    ops.clear_point_orders()
    k = row["k"]
    d = _setup(row, gpu)
    q, s, inds, kp, dk, md = d["q"], d["s"], d["inds"], d["kp"], d["deformed"], d["mod"]
    tmax = R.gaussian_tmax(q, s, inds, kp, EXTENT, dk) if row["influence"] == "gaussian" else 0.0
    rng = np.random.default_rng(7)
    dwf = dmin = None
    if row["bwd"]:
        dwf = rng.standard_normal((q.shape[0], k, row["ci"])).astype(np.float32)
        dmin = rng.standard_normal((q.shape[0], k)).astype(np.float32) if dk is not None else None
    got = _run(row, d, gpu, dwf, dmin)
    ref, ref_min = R.ref_forward(d["x"], q, s, inds, kp, EXTENT, row["influence"], row["aggregation"], dk, md)
    tol = R.fwd_bound(d["x"], q, s, inds, kp, EXTENT, row["influence"], row["aggregation"], dk, md, tmax, ref, False)
    GB._check(got["wf"], ref, tol, "wf")
    if dk is not None:
        GB._check(got["min_d2"], ref_min, R.min_d2_bound(ref_min, q, s, inds, dk), "min_d2")
    if not row["bwd"]:
        return
    rdx, rdk, rdm = R.ref_backward(d["x"], dwf, q, s, inds, kp, EXTENT, row["influence"], row["aggregation"], dk, md, dmin)
    tol = R.dx_bound(dwf, q, s, inds, kp, EXTENT, row["influence"], row["aggregation"], dk, md, tmax, rdx, False, d["x"].shape)
    GB._check(got["dx"], rdx, tol, "dx")
    if row["queries"] == "hub":
        ns = s.shape[0]
        cnt = np.bincount(inds[inds < ns], minlength=ns)
        assert cnt[ns - 1] >= 300 and (cnt == 0).sum() >= 100, "hub / unreached supports missing"
        assert np.abs(rdx[ns - 1]).max() > 0 and np.all(got["dx"][cnt == 0] == 0)
    if row["geom"]:
        tk, tm = R.geom_bounds(d["x"], dwf, q, s, inds, dk, md, EXTENT, row["influence"], row["aggregation"], dmin)
        GB._check(got["d_dkp"], rdk, tk, "d deformed_kp")
        if md is not None:
            GB._check(got["d_mod"], rdm, tm, "d modulations")


# ------------------------------------------------------------------------------------------------------------------
# K4 packed: four supports per wave, bit-identical to the single-support form (which the rows above hold to float64)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", SIZES)
@pytest.mark.parametrize("ci", [4, 32, 64])
def test_ksize_packed_k4_bit_identical(gpu, k, ci):
    from weasal_amd import _lib, ops
    from weasal_amd._lib import check, current_stream, ptr
    lib = _lib.lib()
    rng = np.random.default_rng(100 * k + ci)
    # a strided layer's shape: fewer queries than supports, ~8 incoming pairs per support, some supports with more than 16
    s = R.lattice_cloud(rng, 1500, 1.0)
    q = R.lattice_cloud(rng, 400, 1.0)
    h = 30
    inds = R.brute_rows(q, s, RADIUS, h)
    inds[:60, :] = np.where(inds[:60, :] < 1500, 7, inds[:60, :])      # support 7: far more than 16 pairs (the whole-wave path)
    kp = R.lattice_kernel(rng, k, KP_REACH)
    Q, S, I = (torch.from_numpy(a).to(gpu) for a in (q, s, inds))
    table = ops.TransposedTable(I, 1500)
    dwf = torch.from_numpy(rng.standard_normal((400, k, ci)).astype(np.float32)).to(gpu)
    KPt = torch.from_numpy(kp).to(gpu)
    buf = C.create_string_buffer(256)
    check(lib.ws_kpconv_gather_bwd_x_packed_variant(400, 1500, h, ci, dwf.data_ptr(), dwf.data_ptr(), 0, 0, 0, 0, 0, 0, buf, 256))
    assert buf.value.decode().startswith(PACKED + "<K=15, ")          # (this reporter answers for K = 15; the plan does not depend on K)
    outs = []
    for name in ("ws_kpconv_gather_bwd_x_packed", "ws_kpconv_gather_bwd_x_gated"):
        dx = torch.full((1500, ci), float("nan"), device=gpu)
        check(getattr(lib, name)(ptr(Q), 400, ptr(S), 1500, ptr(I), h, ptr(table.offsets), ptr(table.pairs), ptr(dwf), ci, ptr(KPt), k,
                                 None, None, EXTENT, 0, 0, None, None, 0.0, ptr(dx), current_stream()))
        outs.append(dx)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    rdx, _, _ = R.ref_backward(np.zeros((1500, ci), np.float32), dwf.cpu().numpy(), q, s, inds, kp, EXTENT)
    tol = R.dx_bound(dwf.cpu().numpy(), q, s, inds, kp, EXTENT, "linear", "sum", ref=rdx, x_shape=(1500, ci))
    GB._check(outs[0].cpu().numpy(), rdx, tol, "dx (packed)")


# ------------------------------------------------------------------------------------------------------------------
# K4G: the table-free backward on the self-query layers of an activated batch
# ------------------------------------------------------------------------------------------------------------------
def _grid_case(gpu, batch, cfg, lvl, k, ci, variant, wide):
    """GB._grid_case with k kernel points, f32 rows -> (grid-walk dx, index-order dx, table dx, bound of |walk - table|)"""
    from weasal_amd import _lib, ops
    sorted_switch = C.c_int.in_dll(_lib.lib(), "ws_kpconv_grid_sorted")
    p, inds = batch.points[lvl], batch.neighbors[lvl]
    grid = ops._grid_for(inds)
    assert grid is not None and grid.ns == p.shape[0]
    assert (grid.max_count > ops.GRID_NARROW_MAX) == wide, (grid.max_count, wide)
    r = cfg.first_subsampling_dl * cfg.conv_radius * 2 ** lvl
    extent = r * cfg.KP_extent / cfg.conv_radius
    gen = torch.Generator(device=gpu).manual_seed(ci * 7 + lvl + 1000 * k)
    kp = torch.randn(k, 3, device=gpu, generator=gen) * (0.6 * r)
    kw = {}
    if variant == "deformable":
        kw = dict(deformed_kp=kp[None] + 0.1 * r * torch.randn(p.shape[0], k, 3, device=gpu, generator=gen),
                  modulations=torch.rand(p.shape[0], k, device=gpu, generator=gen), want_min_d2=True)
    elif variant == "gaussian-closest":
        kw = dict(influence="gaussian", aggregation="closest")
    dwf = torch.randn(p.shape[0], k, ci, device=gpu, generator=gen)
    ordered = ops._order_for(p) is not None
    dx_like = torch.empty(p.shape[0], ci, device=gpu)

    def asked(sort):
        kernel, args, keys = report("bwd_x_grid_wide" if wide else "bwd_x_grid", k, p.shape[0], p.shape[0], ci, dwf.data_ptr(),
                                    dx_like.data_ptr(), deformed=variant == "deformable", modulated=variant == "deformable",
                                    influence=kw.get("influence", "linear"), aggregation=kw.get("aggregation", "sum"), ordered=ordered)
        want = GB.grid_plan(ci, variant, "f32", wide, sort, ordered)
        want_args = dict(GB.table_launch(*want[:2])[1], K=str(k))
        assert (kernel, args, keys["ilv"]) == (want[0], want_args, want[2]), (kernel, args, keys)
    try:
        sorted_switch.value = 1
        asked(True)
        idx_order = GB._grid_dx(p, inds, dwf, kp, extent, kw, True, torch.float32)
        sorted_switch.value = 0
        asked(False)
        walk = GB._grid_dx(p, inds, dwf, kp, extent, kw, True, torch.float32)
        table = GB._grid_dx(p, inds, dwf, kp, extent, kw, False, torch.float32)
        mag = GB._grid_dx(p, inds, dwf.abs(), kp, extent, kw, False, torch.float32)
        mag1 = GB._grid_dx(p, inds, dwf.abs(), kp, extent, dict(influence="constant"), False, torch.float32)
    finally:
        sorted_switch.value = 0
        ops.GRID_BACKWARD = True
    assert int(grid.overflow.item()) == 0
    ns = p.shape[0]
    flat = inds.reshape(-1)
    n = float(k) * torch.bincount(flat[flat < ns], minlength=ns)[:ns].double() + 6.0
    tmax = 0.0
    if variant == "gaussian-closest":
        real = inds < ns
        nb = (p.double()[inds.clamp(max=ns - 1)] - p.double()[:, None, :])[real]
        d2 = ((nb[:, None, :] - kp.double()[None]) ** 2).sum(-1)
        tmax = float(d2.max()) / (2 * (float(np.float32(extent)) * 0.3) ** 2)
    c1, c2 = R.weight_constants("gaussian" if variant == "gaussian-closest" else "linear", tmax)
    tol = 2 * (n[:, None] + c1) * R.U * mag.double() + 2 * c2 * R.U * mag1.double()
    return walk, idx_order, table, tol


@pytest.mark.parametrize("k", SIZES)
@pytest.mark.parametrize("ci,variant", [(4, "rigid"), (3, "rigid"), (8, "gaussian-closest"), (16, "deformable"), (32, "rigid"),
                                        (30, "deformable"), (64, "rigid"), (50, "gaussian-closest")])
def test_ksize_grid_backward_slab_vs_table(gpu, k, ci, variant):
    """K4G slab form at K = 9 / 13, every G, MODE 0 / 1, float4 and scalar rows, SORT on and off"""
    cfg, batch = GB._slab_batch(gpu)
    batch.activate()
    for lvl in (0, 2):
        walk, idx_order, table, tol = _grid_case(gpu, batch, cfg, lvl, k, ci, variant, False)
        assert torch.equal(idx_order, table), (lvl, float((idx_order - table).abs().max()))
        msg = R.describe(walk.cpu().numpy(), table.cpu().numpy(), tol.cpu().numpy(), "dx level %d" % lvl)
        assert not msg, msg


@pytest.mark.parametrize("k", SIZES)
@pytest.mark.parametrize("ci", [4, 30, 64, 128, 256])
def test_ksize_grid_backward_wide_vs_table(gpu, k, ci):
    """K4G wide form (MODE 0) at K = 9 / 13: G = 1 / 8 / 16, NCH 1 / 2 / 4"""
    cfg, batch = GB._wide_batch(gpu)
    batch.activate()
    walk, idx_order, table, tol = _grid_case(gpu, batch, cfg, 0, k, ci, "rigid", True)
    msg = R.describe(walk.cpu().numpy(), table.cpu().numpy(), tol.cpu().numpy(), "dx")
    assert not msg, msg


# ------------------------------------------------------------------------------------------------------------------
# the element-wise ends (deform.hip) at K = 9 / 13 against oracle/deform_ref.py.  The restatement reads its kernel size from
# the module attribute K; the constants of its summation bounds (15 terms per thread, 14 partners per point) stay those of
# K = 15: upper bounds of the smaller sizes' counts.
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", SIZES)
@pytest.mark.parametrize("n,modulated", [(1, True), (17, False), (1000, True)])
def test_ksize_deform_prepare_vs_float64(gpu, monkeypatch, k, n, modulated):
    from weasal_amd import _lib, ops
    monkeypatch.setattr(D, "K", k)
    assert (n * k) % 256
    rng = np.random.default_rng(100 + n + k)
    kp = (rng.standard_normal((k, 3)) * 0.3).astype(np.float32)
    off = rng.standard_normal((n, (4 if modulated else 3) * k)).astype(np.float32)
    if modulated:
        off[:, 3 * k:] *= 3.0
    extent = 1.2
    ref, tol = D.prepare_ref(off, kp, extent, modulated)
    O = torch.from_numpy(off).to(gpu).requires_grad_(True)
    kp4, dkp, mod, rmax = ops.deform_prepare(O, torch.from_numpy(kp).to(gpu), extent, modulated)
    g4 = kp4.detach().cpu().numpy()
    GB._check(g4, ref, tol, "kp4")
    assert np.array_equal(dkp.detach().cpu().numpy(), g4[..., :3])
    assert (mod is None) == (not modulated) and (mod is None or np.array_equal(mod.cpu().numpy(), g4[..., 3]))
    norm = float(np.sqrt((g4[..., :3].astype(np.float64) ** 2).sum(-1)).max())
    assert norm * (1 - 4 * D.U) <= float(rmax) <= norm * (1 + 4 * D.U)
    d4 = rng.standard_normal((n, k, 4)).astype(np.float32)
    d3 = rng.standard_normal((n, k, 3)).astype(np.float32)
    for second in (None, d3):
        O.grad = None
        outs, grads = [kp4], [torch.from_numpy(d4).to(gpu)]
        if second is not None:
            outs, grads = outs + [dkp], grads + [torch.from_numpy(second).to(gpu)]
        torch.autograd.backward(outs, grads, retain_graph=True)
        rg, rt = D.prepare_bwd_ref(off, d4, second, extent, modulated, tol[..., 3])
        GB._check(O.grad.cpu().numpy(), rg, rt, "d_off")
    # a column count of another size is refused
    with pytest.raises(_lib.WeasalHipError):
        ops.deform_prepare(torch.zeros((n, 45), device=gpu), torch.from_numpy(kp).to(gpu), extent, False)


@pytest.mark.parametrize("k", SIZES)
@pytest.mark.parametrize("n", [1, 257, 3000])
def test_ksize_p2p_regularizer_vs_float64(gpu, monkeypatch, k, n):
    from weasal_amd import ops
    monkeypatch.setattr(D, "K", k)
    rng = np.random.default_rng(40 + n + k)
    extent, rep = 1.2, 1.2
    dkp = (rng.standard_normal((n, k, 3)) * 1.1).astype(np.float32)
    while True:                 # redraw the points that hold a pair within the margin of repulse_extent
        close = D.repulse_margins(dkp, extent, rep) <= 1e-5
        if not close.any():
            break
        dkp[close] = (rng.standard_normal((int(close.sum()), k, 3)) * 1.1).astype(np.float32)
    md = np.abs(rng.standard_normal((n, k))).astype(np.float32)
    Dk = torch.from_numpy(dkp).to(gpu).requires_grad_(True)
    Md = torch.from_numpy(md).to(gpu).requires_grad_(True)
    out = ops.p2p_regularizer(Dk, Md, extent, rep)
    ref, tol = D.regularizer_ref(dkp, md, extent, rep)
    GB._check(out.detach().cpu().numpy(), ref, tol, "regularizer")
    g = np.array([0.7, -1.3], np.float32)
    out.backward(torch.from_numpy(g).to(gpu))
    rk, tk, rm, tm = D.regularizer_bwd_ref(dkp, md, extent, rep, g)
    GB._check(Dk.grad.cpu().numpy(), rk, tk, "regularizer d_kp")
    GB._check(Md.grad.cpu().numpy(), rm, tm, "regularizer d_min_d2")
