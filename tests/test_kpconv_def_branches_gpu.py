"""Every launch branch of the deformable fast path held to a float64 reference, per element: the MODE-2 instantiations of
kpconv_gather_fwd_mfma_kernel and kpconv_gather_bwd_x_kernel, MODE 2 of kpconv_gather_bwd_x_gridw_kernel, the matrix-core
geometry backward kpconv_gather_bwd_geom_def_kernel (weasal_amd/csrc/kpconv.hip) and the element-wise ends in deform.hip.

The harness is the one of tests/test_kpconv_branches_gpu.py (rows `_b`, `report` / `parse_launch`, `_setup`, the lattice
geometry and the bounds of oracle/kpconv_branch_ref.py); `DEF_BRANCHES` is the table of this family.  Each row names what
ops.kpconv_gather_def launches for it: forward (ws_kpconv_gather_fwd_def), dx through the transposed table
(ws_kpconv_gather_bwd_x_def) and, where kp4 asks for its gradient, the geometry backward (ws_kpconv_gather_bwd_geom_def).
Before anything is launched ws_kpconv_gather_variant is asked with the device pointers of the run and has to name them
(tests/test_kpconv_branches_cpu.py asks it about every row with stand-in addresses).  The rules behind the rows:
  forward   fwd_def_plan: NT from ci as in the generic forward (<=16: 1, <=32: 2, <=64: 4, <=128: 8, else 16), NT = 1 unless
            ci % NT == 0 and the rows are 16-byte aligned; no SPLIT_NT narrowing, no csplit; CUT = rows_sorted; bf16 rows with
            NT = 1 need an even ci.  (ci = 20 keeps NT = 2 -- one partial 32-channel block; ci = 100 falls back to NT = 1 and
            loops 7 blocks; 48, 80, 96, 192 and 384 end in a partial block whose lanes past ci are masked.)
  dx        bwd_x_plan with MODE 2: G from ci (<=4: 1, <=8: 2, <=16: 4, <=32: 8, else 16), VEC = ci % 4 == 0 and aligned
            dwf / dx; bf16 rows have no scalar form (refused).
  geometry  bwd_geom_def_plan: ci % 16 == 0 and 16-byte aligned x / dwf, or refused; AREG for ci in (16, 32, 64, 128) with
            CK = ci / 4, else CK = 32 / 16 / 8 / 4 by the largest of 128 / 64 / 32 / 16 dividing ci, ci / (4 CK) passes; CUT =
            rows_sorted.
  queue     bwd_x_gridw_plan with MODE 2 (the packed caller takes it at any row width): G as above, VEC, NCH (G = 16 only:
            <=64: 1, <=128: 2, else 4), ilv = GRID_INTERLEAVE with a point order on the supports.
Unreachable, so in no row: kpconv_gather_bwd_x_kernel / _gridw_kernel<MODE 2, VEC = false, bf16> (rows_vec4_or_f32 refuses
bf16 rows that are not 8-byte aligned 4-channel pieces); the gridw form with NCH > 1 below G = 16.  A bf16 x that is only
2-byte aligned is accepted by the forward: NT = 1 moves single elements (RowLoad<1, bf16_t>: ld1 / st1), every access
naturally aligned -- the row `view_offset_bf16` runs it.

Inputs: kp4 [nq, 15, 4] is built by hand -- xyz from R.lattice_deformed (every squared distance exact in f32, the extent
margin asserted), the modulation column uniform in [0.25, 2] with exact zeros (wf and d xyz vanish there, d modulation does
not).  Reference: R.ref_forward / R.ref_backward with deformed = kp4[..., :3], mod = kp4[..., 3], linear, sum.  Bounds:
R.fwd_bound, R.dx_bound, R.geom_bounds, R.min_d2_bound -- the constants of the generic kernels hold for MODE 2 (derived
in the oracle's docstring).  Sorted-row cases (`cut`): rows of three lengths (<= 64, 65..128, > 128 real columns),
kernel points of every fourth query moved out by the search radius, queries whose reach ends inside the second and inside
the third chunk, queries in a void beyond every influence; the counts of each (R.cutoff_counts) are asserted in float64; the results are held to the same
bounds and are equal, bit for bit, to the rows_sorted = False run (the skipped terms are exact zeros of the same
summation split).

test_grid_backward_def_vs_table holds the queue form to the table form (which the rows above hold to float64), with and
without a kp_rmax from the caller; test_grid_backward_def_kp_rmax_bit_identical asks for equal bits between those two (the
entry takes the maximum itself when none is passed); test_deform_prepare_* / test_p2p_regularizer_* hold deform.hip to
oracle/deform_ref.py.
"""
import zlib

import numpy as np
import pytest
import torch

import test_kpconv_branches_gpu as GB
from oracle import deform_ref as D
from oracle import kpconv_branch_ref as R

pytestmark = pytest.mark.gpu

K = GB.K
EXTENT = GB.EXTENT
GD = "kpconv_gather_bwd_geom_def_kernel"
CUT_RADIUS = 1.0        # search radius of the sorted-row cases: well beyond max |kp| + extent (about 0.7)
CUT_H = 200
CUT_VOID = 40           # queries placed in a void: their nearest support is beyond every influence
CUT_ENDS = 10           # at least this many queries whose walk the cutoff ends inside the second chunk, and inside the third


def _tb(v):
    return "true" if v else "false"


def _gd(ck, areg, t, cut=False):
    return (GD, "CK=%d, AREG=%s, T=%s, CUT=%s" % (ck, _tb(areg), t, _tb(cut)))


def fwd_nt(ci, aligned=True):
    nt = 1 if ci <= 16 else 2 if ci <= 32 else 4 if ci <= 64 else 8 if ci <= 128 else 16
    return nt if (ci % nt == 0 and (nt == 1 or aligned)) else 1


def geom_ck(ci):
    """(CK, AREG) of bwd_geom_def_plan, None where it refuses"""
    if ci % 16:
        return None
    if ci in (16, 32, 64, 128):
        return ci // 4, True
    return (32 if ci % 128 == 0 else 16 if ci % 64 == 0 else 8 if ci % 32 == 0 else 4), False


def _d(id, ci, nq, nt, geom, dtype="f32", h=None, queries="self", rows_sorted=False, view="aligned", vec=None, order=False,
       cut=False, refuse=(), note=""):
    """one row: nt = the forward's NT, geom = (CK, AREG) or None (kp4 without requires_grad), vec = VEC of K4 (default: ci % 4
    == 0), refuse = the entries expected to refuse ("fwd", "dx", "geom")"""
    t = GB._tn(dtype)
    vec = (ci % 4 == 0) if vec is None else vec
    row = GB._b(id, "ws_kpconv_gather_fwd_def", GB.MF, GB._mf(nt, 2, True, t, cut=rows_sorted), ci, nq, h=h, dtype=dtype,
                deform="def", rows_sorted=rows_sorted, view=view, queries=queries, bwd=GB._k4(GB._k4g(ci), 2, vec, t),
                geom=_gd(geom[0], geom[1], t, rows_sorted) if geom else None, order=order, note=note)
    row["cut"] = cut
    row["refuse"] = tuple(refuse)
    return row


DEF_BRANCHES = []
for _dt in ("f32", "bf16"):
    DEF_BRANCHES += [
        # ---- the channel ladder: every NT, every (CK, AREG)
        _d("def_ci16_" + _dt, 16, 600, 1, (4, True), _dt),
        _d("def_ci32_" + _dt, 32, 600, 2, (8, True), _dt),
        _d("def_ci64_" + _dt, 64, 500, 4, (16, True), _dt),
        _d("def_ci128_" + _dt, 128, 400, 8, (32, True), _dt),
        _d("def_ci256_" + _dt, 256, 300, 16, (32, False), _dt, note="two passes of the product"),
        _d("def_ci48_" + _dt, 48, 400, 4, (4, False), _dt, note="three passes; partial 64-channel block"),
        _d("def_ci80_" + _dt, 80, 400, 8, (4, False), _dt, note="five passes; partial 128-channel block"),
        _d("def_ci96_" + _dt, 96, 400, 8, (8, False), _dt, note="three passes; partial 128-channel block"),
        _d("def_ci192_" + _dt, 192, 300, 16, (16, False), _dt, note="three passes; partial 256-channel block"),
        _d("def_ci384_" + _dt, 384, 200, 16, (32, False), _dt, note="three passes; a full and a partial 256-channel block"),
        # ---- forward + dx only: the geometry backward refuses ci % 16 != 0
        _d("def_ci20_" + _dt, 20, 400, 2, None, _dt, refuse=("geom",), note="one partial 32-channel block"),
        _d("def_ci100_" + _dt, 100, 400, 1, None, _dt, refuse=("geom",), note="NT falls back: 7 blocks looped"),
        # ---- scheduling orders on queries and supports: bit-identical to the unordered run
        _d("def_order_" + _dt, 32 if _dt == "f32" else 64, 500, 2 if _dt == "f32" else 4, (8, True) if _dt == "f32" else (16, True),
           _dt, queries="distinct", order=True),
        # ---- fewer queries than the waves of a workgroup
        _d("def_nq1_" + _dt, 32, 1, 2, (8, True), _dt, queries="distinct"),
        _d("def_nq3_" + _dt, 64, 3, 4, (16, True), _dt, queries="distinct"),
    ]
    # ---- sorted rows (CUT): every NT, every (CK, AREG)
    for _ci in (16, 32, 64, 128, 256, 48, 96, 192):
        DEF_BRANCHES.append(_d("def_cut_ci%d_%s" % (_ci, _dt), _ci, 280 if _ci < 192 else 200, fwd_nt(_ci), geom_ck(_ci), _dt,
                               h=CUT_H, queries="distinct", rows_sorted=True, cut=True))
# ---- K4 MODE 2 across the G ladder and VEC, on the rows where one support has several hundred incoming pairs
for _ci in (4, 3, 8, 6, 16, 14, 32, 30, 64, 50):
    for _dt in ("f32", "bf16") if _ci % 4 == 0 else ("f32",):
        DEF_BRANCHES.append(_d("def_k4_g%d_%s_ci%d_%s" % (GB._k4g(_ci), "vec" if _ci % 4 == 0 else "scalar", _ci, _dt), _ci, 400,
                               fwd_nt(_ci), None, _dt, h=40, queries="hub", refuse=("geom",) if _ci % 16 else ()))
# ---- row widths: the edges of a 16-neighbour block, of nblk and of a 64-column chunk; rows that are all shadow
for _h in (1, 15, 16, 17, 63, 64, 65, 129, 200):
    DEF_BRANCHES.append(_d("def_width_h%d_f32" % _h, 32, 300, 2, (8, True), "f32", h=_h, queries="dense"))
    DEF_BRANCHES.append(_d("def_width_h%d_bf16" % _h, 64, 300, 4, (16, True), "bf16", h=_h, queries="dense"))
DEF_BRANCHES += [
    # ---- row views.  f32 x = flat[1:] and a dwf 4 bytes off alignment too: NT = 1, scalar K4, no geometry backward
    _d("def_view_offset_f32", 32, 400, 1, None, "f32", view="offset", vec=False, refuse=("geom",),
       note="2 blocks looped; dwf = flat[1:] as well"),
    # a bf16 x 2 bytes off: NT = 1 moves single bf16 elements; dwf / dx are fresh allocations (8-byte pieces)
    _d("def_view_offset_bf16", 32, 400, 1, None, "bf16", view="offset", refuse=("geom",)),
    # ---- refusals (nothing launched by the refused entry)
    _d("def_refuse_bf16_odd", 17, 200, 1, None, "bf16", refuse=("fwd", "dx", "geom"), note="bf16 rows need an even ci"),
    _d("def_refuse_bf16_ci18_dx", 18, 200, 2, None, "bf16", refuse=("dx", "geom"), note="forward runs; dx needs ci % 4 == 0"),
]


# ------------------------------------------------------------------------------------------------------------------
# the reporter on a row
# ------------------------------------------------------------------------------------------------------------------
def check_def_plan(row, ptr, nq, ns, rows_sorted=None):
    """ws_kpconv_gather_variant names what the row says its three entries launch, or refuses where the row says so.
    ptr(name) -> address of x / wf / dwf / dx; -> the plans it answered, as test_kpconv_branches_cpu._plan_key wants them"""
    from weasal_amd import _lib
    srt = row["rows_sorted"] if rows_sorted is None else rows_sorted
    answered = []
    for what, op, a, b, want in (("fwd", "fwd_def", "x", "wf", (row["kernel"], row["targs"])),
                                 ("dx", "bwd_x_def", "dwf", "dx", row["bwd"]),
                                 ("geom", "bwd_geom_def", "x", "dwf", row["geom"])):
        ask = lambda: GB.report(op, nq, ns, row["ci"], ptr(a), ptr(b), dtype=row["dtype"], deformed=True, modulated=True,
                                rows_sorted=srt, ordered=row["order"])
        if what in row["refuse"]:
            with pytest.raises(_lib.WeasalHipError):
                ask()
            continue
        if want is None:
            continue
        kernel, args, keys = ask()
        k_want, a_want, _ = GB.table_launch(*want)
        if "CUT" in a_want:
            a_want = dict(a_want, CUT=_tb(srt))
        assert (kernel, args) == (k_want, a_want), (row["id"], what, kernel, args)
        assert what != "fwd" or keys["csplit"] == 1
        answered.append((kernel, args, keys))
    return answered


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------
def _modulations(rng, nq):
    """[nq, K] f32 in [0.25, 2] with exact zeros on about a tenth of the entries"""
    mod = rng.uniform(0.25, 2.0, size=(nq, K)).astype(np.float32)
    mod[rng.random((nq, K)) < 0.1] = 0.0
    return mod


def setup_cut(row):
    """distance-sorted rows of width CUT_H from a search radius far beyond every influence.  Row lengths: queries i % 3 == 0
    keep 48 columns, i % 3 == 1 keep 100, the rest all (about 200).  Kernel points: i % 4 == 0 has three of them moved out by
    the search radius (their minimum is found far down the row, the whole row is walked); i % 4 == 1 has a kernel of
    half the size with one point 0.26 out (the walk ends inside the second chunk); i % 4 == 3 one point 0.38 out (it ends
    inside the third).  The last CUT_VOID queries sit 50 lattice steps outside the cloud."""
    rng = np.random.default_rng(zlib.crc32(row["id"].encode()))
    nq = row["nq"]
    nreg = nq - CUT_VOID
    kp = R.lattice_kernel(rng, K, GB.KP_REACH)
    kp_small = R.lattice_kernel(rng, K, 0.5 * GB.KP_REACH)
    s = R.lattice_cloud(rng, 3200, 1.5)
    q = R.lattice_cloud(rng, nq, 0.5)
    q[nreg:, 0] = 1.5 + 50 * R.STEP
    ns = s.shape[0]
    inds = R.brute_rows(q, s, CUT_RADIUS, CUT_H)
    inds[0:nreg:3, 48:] = ns
    inds[1:nreg:3, 100:] = ns
    deformed = R.lattice_deformed(rng, kp, nq, 0.05)
    small = np.arange(1, nreg, 4)
    deformed[small] = R.lattice_deformed(rng, kp_small, len(small), 0.05)
    # the farthest kernel point decides the reach max |kp| + extent: 16 lattice steps out on the small kernels (reach about
    # 0.56, near column 90 of these rows), 24 steps on every other full-size one (about 0.68, near column 160)
    for group, steps in ((small, 16), (np.arange(3, nreg, 4), 24)):
        deformed[group, 0] = np.float32(R.KP_SHIFT)
        deformed[group, 0, group % 3] += np.float32(steps * R.STEP)
    far = np.arange(0, nreg, 4)
    for j in range(3):
        deformed[far, (far // 4 + 5 * j) % K, j] += np.float32(64 * R.STEP)
    assert R.extent_margin(q, s, inds, kp, EXTENT, deformed) > 1e-6
    x = rng.standard_normal((ns, row["ci"])).astype(np.float32)
    if row["dtype"] == "bf16":
        x = torch.from_numpy(x).bfloat16().float().numpy()
    real = (inds < ns).sum(1)
    assert (real[:nreg] <= 64).sum() >= 20 and ((real[:nreg] > 64) & (real[:nreg] <= 128)).sum() >= 20 and (real > 128).sum() >= 20
    counts = R.cutoff_counts(q, s, inds, deformed, EXTENT)
    print("CUTCASE %s last-influential>=64: %d  argmin>=64 pairs: %d  first-beyond-reach: %d  walk ends in chunk 2: %d  in chunk 3: %d"
          % ((row["id"],) + counts))
    assert min(counts[:3]) >= 20, counts
    assert min(counts[3:]) >= CUT_ENDS, counts
    return dict(q=q, s=s, inds=inds, kp=kp, deformed=deformed, mod=None, x=x)


def setup_def(row, gpu):
    d = setup_cut(row) if row["cut"] else GB._setup(row, gpu)
    d["mod"] = _modulations(np.random.default_rng(zlib.crc32(row["id"].encode()) + 1), d["q"].shape[0])
    assert (d["mod"] == 0).sum() >= 1 or d["q"].shape[0] < 3
    d["kp4"] = np.concatenate([d["deformed"], d["mod"][..., None]], -1).astype(np.float32)
    return d


def _offset_view(t, gpu):
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=gpu)
    flat[1:].copy_(t.reshape(-1))
    v = flat[1:].view(t.shape)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def run_def(row, d, gpu, dwf=None, dmin=None, want_geom=False, rows_sorted=None, ordered=False, kp4_np=None):
    from weasal_amd import ops
    srt = row["rows_sorted"] if rows_sorted is None else rows_sorted
    Q = torch.from_numpy(d["q"]).to(gpu)
    S = Q if row["queries"] == "self" else torch.from_numpy(d["s"]).to(gpu)
    if ordered:
        ops.register_point_order(Q, torch.from_numpy(np.random.default_rng(3).permutation(Q.shape[0]).astype(np.int32)).to(gpu))
        ops.register_point_order(S, torch.from_numpy(np.random.default_rng(4).permutation(S.shape[0]).astype(np.int32)).to(gpu))
        assert ops._order_for(Q) is not None and ops._order_for(S) is not None
    inds = torch.from_numpy(d["inds"]).to(gpu)
    X = GB._gpu_x(d["x"], row["dtype"], row["view"], gpu)
    G = None
    if dwf is not None:
        G = torch.from_numpy(dwf).to(gpu).to(X.dtype)
        if row["view"] == "offset" and row["dtype"] == "f32":
            G = _offset_view(G, gpu)
    bufs = dict(x=X, wf=torch.empty((Q.shape[0], K, row["ci"]), dtype=X.dtype, device=gpu), dx=torch.empty_like(X),
                dwf=G if G is not None else torch.empty((Q.shape[0], K, row["ci"]), dtype=X.dtype, device=gpu))
    check_def_plan(dict(row, order=ordered), lambda name: bufs[name].data_ptr(), Q.shape[0], S.shape[0], srt)
    kp4 = torch.from_numpy(d["kp4"] if kp4_np is None else kp4_np).to(gpu).requires_grad_(want_geom)
    if dwf is not None:
        X = X.detach().requires_grad_(True)
    wf, mn = ops.kpconv_gather_def(X, kp4, Q, S, inds, EXTENT, None, srt)
    out = dict(wf=wf.detach().float().cpu().numpy(), min_d2=mn.detach().cpu().numpy())
    if dwf is not None:
        seen = []
        wf.register_hook(lambda g: seen.append(g.data_ptr()))
        torch.autograd.backward([wf, mn], [G, torch.from_numpy(dmin).to(gpu)])
        assert seen == [G.data_ptr()], "the backward was not handed the dwf the plan was checked with"
        out["dx"] = X.grad.float().cpu().numpy()
        if want_geom:
            out["d_kp4"] = kp4.grad.cpu().numpy()
    torch.cuda.synchronize()
    return out


def held(got, ref, tol, what, row_id):
    """print the worst ratio |got - ref| / bound and the number of elements, then assert the bound element by element"""
    worst, n = R.worst_ratio(got, ref, tol)
    print("RATIO %s %s worst=%.4g n=%d" % (what.replace(" ", "_"), row_id, worst, n))
    msg = R.describe(got, ref, tol, what)
    assert not msg, msg


# ------------------------------------------------------------------------------------------------------------------
# 1. MODE-2 rows against float64
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", DEF_BRANCHES, ids=[r["id"] for r in DEF_BRANCHES])
def test_def_branch_vs_float64(row, gpu):
    from weasal_amd import _lib, ops
    ops.clear_batch_hints()
    ops.clear_point_orders()
    d = setup_def(row, gpu)
    bf = row["dtype"] == "bf16"
    q, s, inds, kp, dk, md = d["q"], d["s"], d["inds"], d["kp"], d["deformed"], d["mod"]
    rng = np.random.default_rng(7)
    dwf = rng.standard_normal((q.shape[0], K, row["ci"])).astype(np.float32)
    if bf:
        dwf = torch.from_numpy(dwf).bfloat16().float().numpy()
    dmin = rng.standard_normal((q.shape[0], K)).astype(np.float32)
    want_geom = row["geom"] is not None
    if "fwd" in row["refuse"]:
        with pytest.raises(_lib.WeasalHipError):
            run_def(row, d, gpu)
        return
    run_bwd = "dx" not in row["refuse"]
    try:
        got = run_def(row, d, gpu, dwf if run_bwd else None, dmin, want_geom, ordered=row["order"])
        if row["order"]:
            ops.clear_point_orders()
            plain = run_def(row, d, gpu, dwf, dmin, want_geom)
            for key in plain:
                assert np.array_equal(plain[key], got[key]), "%s changed under a scheduling order" % key
        if row["cut"]:
            walked = run_def(row, d, gpu, dwf, dmin, want_geom, rows_sorted=False)
            for key in ("wf", "min_d2", "d_kp4", "dx"):
                assert np.array_equal(walked[key], got[key]), "%s differs between the cutoff and the full walk" % key
    finally:
        ops.clear_point_orders()

    ref, ref_min = R.ref_forward(d["x"], q, s, inds, kp, EXTENT, "linear", "sum", dk, md)
    held(got["wf"], ref, R.fwd_bound(d["x"], q, s, inds, kp, EXTENT, "linear", "sum", dk, md, 0.0, ref, bf), "wf", row["id"])
    assert np.all(got["wf"][md == 0] == 0), "a zero modulation leaves a zero row"
    held(got["min_d2"], ref_min, R.min_d2_bound(ref_min, q, s, inds, dk), "min_d2", row["id"])
    if not run_bwd:
        # the forward ran; the transposed-table backward refuses this row type
        X = GB._gpu_x(d["x"], row["dtype"], row["view"], gpu).requires_grad_(True)
        wf, mn = ops.kpconv_gather_def(X, torch.from_numpy(d["kp4"]).to(gpu), torch.from_numpy(q).to(gpu), torch.from_numpy(q).to(gpu),
                                       torch.from_numpy(inds).to(gpu), EXTENT)
        with pytest.raises(_lib.WeasalHipError):
            wf.backward(torch.from_numpy(dwf).to(gpu).to(wf.dtype))
        return
    rdx, rdk, rdm = R.ref_backward(d["x"], dwf, q, s, inds, kp, EXTENT, "linear", "sum", dk, md, dmin)
    held(got["dx"], rdx, R.dx_bound(dwf, q, s, inds, kp, EXTENT, "linear", "sum", dk, md, 0.0, rdx, bf, d["x"].shape), "dx", row["id"])
    if row["queries"] == "hub":
        ns = s.shape[0]
        cnt = np.bincount(inds[inds < ns], minlength=ns)
        assert cnt[ns - 1] >= 300 and (cnt == 0).sum() >= 100, "hub / unreached supports missing"
        assert np.abs(rdx[ns - 1]).max() > 0 and np.all(got["dx"][cnt == 0] == 0)
    if want_geom:
        tk, tm = R.geom_bounds(d["x"], dwf, q, s, inds, dk, md, EXTENT, "linear", "sum", dmin)
        held(got["d_kp4"][..., :3], rdk, tk, "d_kp4 xyz", row["id"])
        held(got["d_kp4"][..., 3], rdm, tm, "d_kp4 w", row["id"])
        if q.shape[0] >= 100:
            assert np.abs(rdm[md == 0]).max() > 0, "d modulation is live where the modulation is zero"
    elif "geom" in row["refuse"]:
        # kp4 asks for its gradient: the matrix-core geometry backward refuses the shape / the view
        X = GB._gpu_x(d["x"], row["dtype"], row["view"], gpu)
        Q = torch.from_numpy(q).to(gpu)
        S = Q if row["queries"] == "self" else torch.from_numpy(s).to(gpu)
        kp4 = torch.from_numpy(d["kp4"]).to(gpu).requires_grad_(True)
        wf, mn = ops.kpconv_gather_def(X, kp4, Q, S, torch.from_numpy(inds).to(gpu), EXTENT)
        with pytest.raises(_lib.WeasalHipError):
            wf.backward(torch.from_numpy(dwf).to(gpu).to(wf.dtype))


def test_def_branch_refuses_wrong_k(gpu):
    """a kernel-point count the build does not instantiate is refused by the forward entry (nothing launched)"""
    from weasal_amd import _lib, ops
    row = DEF_BRANCHES[0]
    d = setup_def(dict(row, nq=50), gpu)
    Q = torch.from_numpy(d["q"]).to(gpu)
    for k in (14, 16):
        kp4 = torch.zeros((Q.shape[0], k, 4), device=gpu)
        with pytest.raises(_lib.WeasalHipError):
            ops.kpconv_gather_def(torch.from_numpy(d["x"]).to(gpu), kp4, Q, Q, torch.from_numpy(d["inds"]).to(gpu), EXTENT)


# ------------------------------------------------------------------------------------------------------------------
# 2. queue form, MODE 2, against the table form
# ------------------------------------------------------------------------------------------------------------------
GRID_DEF_LEVELS = [("slab", 0), ("slab", 1), ("slab", 2), ("wide", 0)]


def grid_def_plan(ci, dt, ordered):
    """(kernel, template arguments, ilv) of ws_kpconv_gather_bwd_x_grid_wide with kp4"""
    return (GB.K4GW, "K=15, G=%d, MODE=2, VEC=%s, NCH=%d, T=%s" % (GB.GRID_G[ci], _tb(ci % 4 == 0), GB.GRID_NCH.get(ci, 1), GB._tn(dt)),
            GB.GRID_ILV if ordered else 0)


def _grid_def_level(gpu, batch, cfg, lvl, ci, bf, queue_only=False):
    """-> (queue dx with the caller's kp_rmax, queue dx without, table dx, bound, row pairs beyond kp_rmax + extent);
    queue_only: the first two and the count alone"""
    from weasal_amd import ops
    p, inds = batch.points[lvl], batch.neighbors[lvl]
    grid = ops._grid_for(inds)
    assert grid is not None and grid.ns == p.shape[0]
    ns = p.shape[0]
    r = cfg.first_subsampling_dl * cfg.conv_radius * 2 ** lvl
    extent = r * cfg.KP_extent / cfg.conv_radius
    gen = torch.Generator(device=gpu).manual_seed(ci * 11 + lvl)
    kp = torch.randn(15, 3, device=gpu, generator=gen)
    kp = kp / kp.norm(dim=1, keepdim=True) * (0.5 * r) * torch.rand(15, 1, device=gpu, generator=gen)
    # offset features whose deformed kernel points reach about 0.9 r for a tenth of the (point, kernel point) pairs
    off = torch.randn(ns, 60, device=gpu, generator=gen) * (0.05 * r / extent)
    push = torch.rand(ns, 15, device=gpu, generator=gen) < 0.1
    dirs = torch.randn(ns, 15, 3, device=gpu, generator=gen)
    dirs = dirs / dirs.norm(dim=2, keepdim=True)
    pushed = (dirs * (0.9 * r) - kp[None]) / extent
    off[:, :45] = torch.where(push[..., None], pushed, off[:, :45].reshape(ns, 15, 3)).reshape(ns, 45)
    off[:, 45:] = torch.randn(ns, 15, device=gpu, generator=gen) * 2
    kp4, _, _, rmax = ops.deform_prepare(off, kp, extent, True)
    kp4 = kp4.detach()
    norms = kp4[..., :3].double().norm(dim=2)
    assert float(norms.max()) > 0.85 * r and float(rmax) >= float(norms.max()) * (1 - 4 * R.U)
    dt = torch.bfloat16 if bf else torch.float32
    dwf = torch.randn(ns, 15, ci, device=gpu, generator=gen).to(dt)
    ordered = ops._order_for(p) is not None
    kernel, args, keys = GB.report("bwd_x_grid_wide", ns, ns, ci, dwf.data_ptr(), torch.empty(ns, ci, device=gpu, dtype=dt).data_ptr(),
                                   dtype="bf16" if bf else "f32", deformed=True, modulated=True, ordered=ordered)
    want = grid_def_plan(ci, "bf16" if bf else "f32", ordered)
    assert (kernel, args, keys["ilv"]) == (want[0], GB.table_launch(*want[:2])[1], want[2]), (kernel, args, keys)

    def dx_of(g, use_grid, rm):
        ops.GRID_BACKWARD = use_grid
        x = torch.zeros(ns, ci, device=gpu, dtype=dt, requires_grad=True)
        wf, _ = ops.kpconv_gather_def(x, kp4, p, p, inds, extent, rm)
        assert ops.dx_route(inds, p, p, "packed")[0] == (ops.QUEUE_GRID if use_grid else ops.TABLE)
        wf.backward(g)
        return x.grad.float()
    # the pairs of the rows that the cutoff decides: farther apart than kp_rmax + extent (float64; the kernel's 1.0001 included)
    real = inds < ns
    dist = (p.double()[inds.clamp(max=ns - 1).long()] - p.double()[:, None, :]).norm(dim=2)
    decided = int((real & (dist > (float(rmax) + float(np.float32(extent))) * 1.0001)).sum())
    try:
        queue = dx_of(dwf, True, rmax)
        queue_all = dx_of(dwf, True, None)
        if queue_only:
            return queue.cpu().numpy(), queue_all.cpu().numpy(), None, None, decided
        table = dx_of(dwf, False, rmax)
        mag = dx_of(dwf.abs(), False, rmax)
        mag1 = GB._grid_dx(p, inds, dwf.abs(), kp, extent, dict(influence="constant"), False, dt)
    finally:
        ops.GRID_BACKWARD = True
    assert int(grid.overflow.item()) == 0
    flat = inds.reshape(-1)
    n = 15.0 * torch.bincount(flat[flat < ns], minlength=ns)[:ns].double() + 6.0
    c1, c2 = R.weight_constants("linear")
    tol = 2 * (n[:, None] + c1) * R.U * mag.double() + 2 * c2 * R.U * mag1.double()
    if bf:
        tol = tol + 2.0 ** -7 * table.abs().double()
    return tuple(t.cpu().numpy() for t in (queue, queue_all, table, tol)) + (decided,)


_GRID_DEF = {}          # the arrays of the latest case
_RMAX_DIFF = {}         # (ci, rows) -> {(batch, level): (elements that differ with / without the caller's kp_rmax, elements)}


def _grid_def_results(gpu, ci, rows, queue_only=False):
    """{(batch, level): _grid_def_level}, computed once per case"""
    if (ci, rows) not in _GRID_DEF and not (queue_only and (ci, rows) in _RMAX_DIFF):
        out = {}
        for which, lvl in GRID_DEF_LEVELS:
            cfg, batch = GB._slab_batch(gpu) if which == "slab" else GB._wide_batch(gpu)
            batch.activate()
            out[(which, lvl)] = _grid_def_level(gpu, batch, cfg, lvl, ci, rows == "bf16", queue_only)
        _RMAX_DIFF[(ci, rows)] = {key: (int((v[0] != v[1]).sum()), v[0].size) for key, v in out.items()}
        if not queue_only:
            _GRID_DEF.clear()
            _GRID_DEF[(ci, rows)] = out
    return _GRID_DEF.get((ci, rows))


@pytest.mark.parametrize("ci,rows", GB.GRID_WIDE, ids=["ci%d-%s" % cv for cv in GB.GRID_WIDE])
def test_grid_backward_def_vs_table(gpu, ci, rows):
    """K4G queue form, MODE 2 (kpconv_gather_bwd_x_gridw_kernel<15, G, 2, VEC, NCH, T>), which the packed caller takes at any
    row width: on levels 0-2 of the narrow pyramid and level 0 of the config-5 limits, within the per-element bound of the
    table form -- which walks every pair of the rows, so a live pair lost to the kp_rmax cutoff shows here.  The cutoff
    decides real candidates on the config-5 level (row pairs farther apart than kp_rmax + extent: counted in float64,
    asserted there); on the narrow levels kp_rmax + extent exceeds the search radius and it decides none."""
    for (which, lvl), (queue, queue_all, table, tol, decided) in _grid_def_results(gpu, ci, rows).items():
        print("RMAXDECIDES %s%d-ci%d-%s row pairs beyond kp_rmax + extent: %d" % (which, lvl, ci, rows, decided))
        assert which != "wide" or decided > 0, "the kp_rmax cutoff decides no candidate on the wide level"
        held(queue, table, tol, "dx queue", "%s%d-ci%d-%s" % (which, lvl, ci, rows))
        held(queue_all, table, tol, "dx queue no rmax", "%s%d-ci%d-%s" % (which, lvl, ci, rows))


def test_grid_backward_def_kp_rmax_bit_identical(gpu):
    """The queue form gives the same bits with the kp_rmax of ops.deform_prepare and with kp_rmax = None, over every case of
    test_grid_backward_def_vs_table.

    Why it holds: the cutoff is part of the summation order on the grid-walk path (kpconv_gather_bwd_x_gridw_kernel tests
    `d2 <= cut2` in `member`, so it decides which pairs share a 64-pair batch, and the flush splits each batch's pool evenly
    over the entry slots).  Given kp4 without kp_rmax, ws_kpconv_gather_bwd_x_grid_wide takes max |kp| over kp4 itself with
    the expression of ws_kpconv_deform_prepare -- the same value -- so both calls walk the same candidates in the same
    batches.  (Run alone, the test launches only the two queue forms of each case.)"""
    for ci, rows in GB.GRID_WIDE:
        _grid_def_results(gpu, ci, rows, queue_only=True)
    bad = ["%s level %d ci %d %s: %d of %d elements" % (which, lvl, ci, rows, differ, n)
           for (ci, rows), levels in _RMAX_DIFF.items() for (which, lvl), (differ, n) in levels.items() if differ]
    assert len(_RMAX_DIFF) == len(GB.GRID_WIDE)
    assert not bad, "dx depends on whether the caller passed kp_rmax:\n" + "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------------
# 3. the element-wise ends (deform.hip)
# ------------------------------------------------------------------------------------------------------------------
def _prepare_inputs(n, modulated, seed):
    rng = np.random.default_rng(seed)
    kp = (rng.standard_normal((K, 3)) * 0.3).astype(np.float32)
    off = rng.standard_normal((n, 60 if modulated else 45)).astype(np.float32)
    if modulated:
        off[:, 45:] *= 3.0
    return off, kp


@pytest.mark.parametrize("n", [1, 17, 1000])
@pytest.mark.parametrize("od", [45, 60])
def test_deform_prepare_vs_float64(gpu, n, od):
    """ws_kpconv_deform_prepare / _bwd (n * 15 is no multiple of 256: the tail lanes redo the last element)"""
    from weasal_amd import ops
    assert (n * K) % 256
    modulated = od == 60
    off, kp = _prepare_inputs(n, modulated, 100 + n + od)
    extent = 1.2
    ref, tol = D.prepare_ref(off, kp, extent, modulated)
    O = torch.from_numpy(off).to(gpu).requires_grad_(True)
    kp4, dkp, mod, rmax = ops.deform_prepare(O, torch.from_numpy(kp).to(gpu), extent, modulated)
    g4 = kp4.detach().cpu().numpy()
    held(g4, ref, tol, "kp4", "prepare-n%d-od%d" % (n, od))
    assert np.array_equal(dkp.detach().cpu().numpy(), g4[..., :3])
    assert (mod is None) == (not modulated) and (mod is None or np.array_equal(mod.cpu().numpy(), g4[..., 3]))
    norm = float(np.sqrt((g4[..., :3].astype(np.float64) ** 2).sum(-1)).max())
    print("RATIO kp_rmax prepare-n%d-od%d worst=%.4g n=1" % (n, od, abs(float(rmax) - norm) / (4 * D.U * norm)))
    assert norm * (1 - 4 * D.U) <= float(rmax) <= norm * (1 + 4 * D.U)
    rng = np.random.default_rng(5)
    d4 = rng.standard_normal((n, K, 4)).astype(np.float32)
    d3 = rng.standard_normal((n, K, 3)).astype(np.float32)
    for second in (None, d3):
        O.grad = None
        outs, grads = [kp4], [torch.from_numpy(d4).to(gpu)]
        if second is not None:
            outs, grads = outs + [dkp], grads + [torch.from_numpy(second).to(gpu)]
        torch.autograd.backward(outs, grads, retain_graph=True)
        rg, rt = D.prepare_bwd_ref(off, d4, second, extent, modulated, tol[..., 3])
        held(O.grad.cpu().numpy(), rg, rt, "d_off" + ("" if second is None else "+dkp"), "prepare-n%d-od%d" % (n, od))


def test_deform_prepare_refuses_and_clears(gpu):
    """a wrong column count is refused; the kp_rmax word is cleared by every call (a second call with smaller offsets on the
    same tensor leaves the second maximum)"""
    from weasal_amd import _lib, ops
    from weasal_amd._lib import check, current_stream, ptr
    off, kp = _prepare_inputs(300, True, 9)
    KPt = torch.from_numpy(kp).to(gpu)
    for modulated, bad in ((True, off[:, :45]), (False, off), (True, off[:, :59])):
        with pytest.raises(_lib.WeasalHipError):
            ops.deform_prepare(torch.from_numpy(np.ascontiguousarray(bad)).to(gpu), KPt, 1.2, modulated)
    rmax = torch.full((1,), 123.0, device=gpu)
    kp4 = torch.empty((300, K, 4), device=gpu)
    seen = []
    for scale in (1.0, 0.25):
        O = torch.from_numpy(off * np.float32(scale)).to(gpu)
        check(_lib.lib().ws_kpconv_deform_prepare(ptr(O), 300, 60, ptr(KPt), K, 1.2, 1, None, None, ptr(kp4), ptr(rmax), current_stream()))
        norm = float(kp4[..., :3].double().norm(dim=2).max())
        seen.append(norm)
        assert norm * (1 - 4 * D.U) <= float(rmax) <= norm * (1 + 4 * D.U)
    assert seen[1] < 0.6 * seen[0]


def _reg_inputs(n, seed):
    """deformed kernel points whose normalised pair distances straddle repulse_extent with a margin"""
    rng = np.random.default_rng(seed)
    extent, rep = 1.2, 1.2
    dkp = (rng.standard_normal((n, K, 3)) * 1.1).astype(np.float32)
    while True:                 # redraw the points that hold a pair within the margin
        close = D.repulse_margins(dkp, extent, rep) <= 1e-5
        if not close.any():
            break
        dkp[close] = (rng.standard_normal((int(close.sum()), K, 3)) * 1.1).astype(np.float32)
    md = np.abs(rng.standard_normal((n, K))).astype(np.float32)
    return dkp, md, extent, rep


@pytest.mark.parametrize("n", [1, 255, 257, 3000])
def test_p2p_regularizer_vs_float64(gpu, n):
    """ws_p2p_regularizer_fwd / _bwd against the float64 restatement of models/architectures.py:24-57; the packed (kp4)
    and the plain (deformed_kp) operand give the same bits"""
    from weasal_amd import _lib, ops
    from weasal_amd._lib import check, current_stream, ptr
    dkp, md, extent, rep = _reg_inputs(n, 40 + n)
    assert D.repulse_margins(dkp, extent, rep).min() > 1e-5
    _, d, c, _, _, _, off = D._pairs(dkp, extent, rep)
    assert (c != 0).sum() >= 10 and ((c == 0) & off).sum() >= 10, "pairs on both sides of repulse_extent"
    Dk = torch.from_numpy(dkp).to(gpu).requires_grad_(True)
    Md = torch.from_numpy(md).to(gpu).requires_grad_(True)
    out = ops.p2p_regularizer(Dk, Md, extent, rep)
    ref, tol = D.regularizer_ref(dkp, md, extent, rep)
    held(out.detach().cpu().numpy(), ref, tol, "regularizer", "n%d" % n)
    g = np.array([0.7, -1.3], np.float32)
    out.backward(torch.from_numpy(g).to(gpu))
    rk, tk, rm, tm = D.regularizer_bwd_ref(dkp, md, extent, rep, g)
    held(Dk.grad.cpu().numpy(), rk, tk, "regularizer d_kp", "n%d" % n)
    held(Md.grad.cpu().numpy(), rm, tm, "regularizer d_min_d2", "n%d" % n)
    # the packed operand
    lib = _lib.lib()
    kp4 = torch.cat([Dk.detach(), torch.rand(n, K, 1, device=gpu)], 2).contiguous()
    out4 = torch.empty(2, device=gpu)
    scratch = torch.empty(max(lib.ws_p2p_regularizer_scratch_bytes(n), 16), dtype=torch.uint8, device=gpu)
    check(lib.ws_p2p_regularizer_fwd(None, ptr(kp4), ptr(Md.detach()), n, K, extent, rep, ptr(out4), ptr(scratch), current_stream()))
    G = torch.from_numpy(g).to(gpu)
    d_md, d_dkp = torch.empty_like(Md.detach()), torch.empty_like(Dk.detach())
    check(lib.ws_p2p_regularizer_bwd(None, ptr(kp4), ptr(Md.detach()), n, K, extent, rep, ptr(G), ptr(d_md), ptr(d_dkp), current_stream()))
    assert torch.equal(out4, out.detach()) and torch.equal(d_md, Md.grad) and torch.equal(d_dkp, Dk.grad)
