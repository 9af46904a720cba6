"""GPU: every branch of the block and decoder-step calls (ws_kpblock_fwd / _bwd, ws_upunary_fwd / _bwd;
weasal_amd/csrc/blocks.hip, descriptors filled by weasal_amd/fused.py) against the float64 reference of oracle/block_ref.py.

Each case of oracle.block_ref's table runs through fused._KPBlockFn.apply / fused._UpUnaryFn.apply with a _Geom built the way
fused.simple_block / fused.resnetb_block build it and hand-made GateLink / SkipSlot objects, at the seed the builder chose
(no LeakyReLU pre-activation within four bounds of zero: nothing is masked).  Per tensor

    max |device - ref64|  <=  4 * max |ref32 - ref64|  +  1e-6 * max |ref64|

(oracle/block_ref.py; the ratio of every (case, tensor) is printed and written to block_branches.json in the ignored report
directory the full-width block test keeps its block_gradients.json in: test_block_gradients_gpu.REPORT).  Every
scratch arena is exactly the queried size and poisoned with NaN, 256 bytes fewer are refused, each backward runs twice on
the same saved forward and must repeat its bits, and the predicates that can be observed (the dX route, the gate link, the
skip slot, launch counts where products group or fuse, the pool's byte record) are asserted per case.

A case whose pointer is deliberately misaligned (a weight or the input one float into a larger buffer) states the contract
of the C entries: the call matches the reference, or returns a non-zero status with a message.  The validators the offset
pointer reaches were read first: Lin::in_place refuses the in-place weight (transpose_small_kernel reads scalars), xb_plan
takes gemm_xb_kernel's guarded scalar loads for an unaligned x / b / gate (or refuses a strided b), xty_plan drops its two-wide
loads, max_pool_plan takes the wave-per-row kernels, arg_bytes() the int32 record."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

from oracle import block_ref as B

pytestmark = pytest.mark.gpu

from test_block_gradients_gpu import REPORT as _BLOCK_GRADIENTS_REPORT

OUT = os.path.join(os.path.dirname(_BLOCK_GRADIENTS_REPORT), "block_branches.json")
_DEFAULTS = {"ws_block_gates": 1, "ws_block_packed_k4": 1, "ws_block_pool_order": 1, "ws_block_group_rows": B.NO_LIMIT,
             "ws_block_gather_residual": 1, "ws_block_fused_infer": 1}
_RESULTS = {}


def _dump():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    kinds = {}
    for name, r in _RESULTS.items():
        for k, v in r.get("ratios", {}).items():
            if v["ratio"] > kinds.get(k, ("", -1.0))[1]:
                kinds[k] = (name, v["ratio"])
    with open(OUT, "w") as f:
        json.dump({"bound": "max|dev - ref64| <= %g * max|ref32 - ref64| + %g * max|ref64|" % (B.FACTOR, B.FLOOR),
                   "worst_ratio_per_tensor": {k: {"case": n, "ratio": r} for k, (n, r) in sorted(kinds.items())},
                   "cases": _RESULTS}, f, indent=1, sort_keys=True)


class _Switches:
    """the library's A/B switches at their defaults but for what the case sets; restored on the way out"""

    def __init__(self, values):
        self.values = dict(_DEFAULTS, **values)

    def __enter__(self):
        from weasal_amd import fused
        lib = fused._bind()
        self.cells = {k: (C.c_int64 if k == "ws_block_group_rows" else C.c_int).in_dll(lib, k) for k in self.values}
        self.old = {k: cell.value for k, cell in self.cells.items()}
        self.infer = fused.FUSED_INFER
        for k, v in self.values.items():
            self.cells[k].value = v
        fused.FUSED_INFER = bool(self.values["ws_block_fused_infer"])       # (fused.py sizes the saved `wf` by its own copy)
        return self

    def __exit__(self, *exc):
        from weasal_amd import fused
        for k, v in self.old.items():
            self.cells[k].value = v
        fused.FUSED_INFER = self.infer


class _Scratch:
    """fused._scratch with exactly the queried bytes, filled with NaN; `short`: the call numbers that get 256 bytes fewer"""

    def __init__(self):
        self.sizes, self.short = [], ()

    def __call__(self, nbytes, device):
        n = int(nbytes)
        self.sizes.append(n)
        assert n >= 256 and n % 256 == 0, n
        if len(self.sizes) in self.short:
            n = max(n - 256, 16)
        return torch.full((n // 4,), float("nan"), dtype=torch.float32, device=device).view(torch.uint8)


def _offset_view(t, gpu):
    """t on the device as a contiguous view one float into a larger buffer: 4-byte aligned, never 16"""
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device=gpu)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v.detach()


def _dev(t, gpu):
    return None if t is None else t.to(gpu).contiguous()


def _pyramid_level(gpu):
    """(device geometry, CPU geometry) of one self-query level of pyramid.build_batch that carries a search grid"""
    from weasal_amd import config as wcfg, pyramid, synthetic
    cfg = wcfg.DALESPLConfig()
    pts, feats, labels, lens = synthetic.make_inputs(21, 3, 4000, 4.0, cfg.in_features_dim)
    np.random.seed(8)
    batch = pyramid.build_batch(cfg, torch.from_numpy(pts).to(gpu), torch.from_numpy(feats).to(gpu), torch.from_numpy(labels).to(gpu),
                                lens, [40, 45, 50, 50, 40])
    batch.activate()
    torch.cuda.synchronize()
    levels = []
    for mat, grid in batch.search_grids:
        for l, nb in enumerate(batch.neighbors):
            if nb is mat:
                levels.append((l, batch.points[l].shape[0], grid.max_count))
    fit = [t for t in levels if 48 <= t[1] <= 512 and t[2] <= 128]
    assert fit, "no level of 48 .. 512 rows with a slab grid: (level, rows, widest row) = %s" % (levels,)
    l = min(fit, key=lambda t: abs(t[1] - 200))[0]
    inds, pts_l = batch.neighbors[l], batch.points[l]
    radius = [r for m, r in batch.search_radii if m is inds][0]
    kp = B.kernel_points(15, radius)
    dev = types.SimpleNamespace(q=pts_l, s=pts_l, inds=inds, kp=kp.to(gpu), keep=batch)
    cpu = types.SimpleNamespace(q_pts=pts_l.cpu(), s_pts=pts_l.cpu(), inds=inds.cpu(), kp=kp, extent=0.48 * radius, radius=radius,
                                search_radius=radius)
    return dev, cpu


def _kp_device_geometry(gpu, c, geo):
    from weasal_amd import ops
    s = geo.s_pts.to(gpu)
    q = geo.q_pts.to(gpu) if c.strided else s
    inds = geo.inds.to(gpu).contiguous()
    if c.rows_sorted:
        ops.active_hints().add(inds, radius=geo.search_radius)
    if c.orders:                 # scheduling orders of the two point sets (any permutation: results never depend on it)
        for p in ((s, q) if c.strided else (s,)):
            ops.register_point_order(p, torch.argsort(p[:, 0]).to(torch.int32))
    return types.SimpleNamespace(q=q, s=s, inds=inds, kp=geo.kp.to(gpu))


def _pool_byte_record_ok(lib, c, feat, nq):
    aligned = torch.empty(64, device=feat.device)
    buf = C.create_string_buffer(160)
    return lib.ws_pool_variant(0, nq, c.in_dim, C.c_void_p(feat.data_ptr()), C.c_void_p(aligned.data_ptr()), C.c_void_p(aligned.data_ptr()),
                               0, 1, 1 if c.orders else 0, buf, 160, None) == 0


def _run_kp(gpu, name):
    from weasal_amd import fused, ops
    lib = fused._bind()
    c = B.CASES[name]
    ops.clear_batch_hints()
    if c.geometry == "pyramid":
        dg, geo = _pyramid_level(gpu)
        b = B.build(name, geo)
    else:
        b = B.build(name)
        geo = b.geo
        dg = _kp_device_geometry(gpu, c, geo)
    t = b.inputs
    led = B.ledger(c, h=geo.inds.shape[1])
    res = {"seed": b.seed, "tries": b.tries, "rows": [int(dg.q.shape[0]), int(dg.s.shape[0]), int(dg.inds.shape[1])], "ledger": {k: str(v) for k, v in led.items()}}
    P = {k: _dev(t[k], gpu) for k in ("feat", "w1", "b1", "wk", "bk", "w2", "b2", "ws", "bs")}
    if c.offset:
        P[c.offset] = _offset_view(t[c.offset], gpu)
    for k, v in P.items():
        if v is not None and (k != "feat" or c.want_dfeat) and not c.infer:
            v.requires_grad_(True)
    conv = types.SimpleNamespace(kernel_points=dg.kp, KP_extent=geo.extent, radius=geo.radius)
    scratch, real_scratch = _Scratch(), fused._scratch
    fused._scratch = scratch
    try:
        with _Switches(c.switches), torch.set_grad_enabled(not c.infer):
            g = fused._geometry(conv, dg.q, dg.s, dg.inds, c.strided)
            g.in_dim, g.conv_in, g.conv_out, g.out_dim, g.slope = c.in_dim, c.conv_in, c.conv_out, c.out_dim, B.SLOPE
            assert g.infer == c.infer
            if c.geometry == "cpu":
                assert g.rows_sorted == c.rows_sorted
            res["route"] = g.dx_route
            assert g.dx_route == (ops.SLAB_GRID if led.get("route") == "slab grid" else ops.TABLE)
            if c.kind == "resnet":        # fused.resnetb_block
                if not c.infer and (g.dx_route == ops.TABLE or c.strided):
                    g.table = ops.transposed_table(g.inds, g.s_pts.shape[0])
            elif not c.infer and c.want_dfeat and g.dx_route == ops.TABLE:      # fused.simple_block
                g.table = ops.transposed_table(g.inds, g.s_pts.shape[0])
            slot = li = None
            if c.dfeat_add:
                slot = fused.SkipSlot()
                slot.armed, g.skip_slot = True, slot
            if c.gate_dfeat:
                li = fused.GateLink()
                g.link_in = li
            args = (P["feat"], P["w1"], P["b1"], P["wk"], P["bk"], P["w2"], P["b2"], P["ws"], P["bs"], g)
            torch.cuda.synchronize()
            n0 = lib.ws_launch_count()
            try:
                out = fused._KPBlockFn.apply(*args)
            except RuntimeError as e:
                assert c.offset and len(str(e)) > 20, (name, str(e))      # the misaligned contract: a status and a message
                res["refused"] = str(e)
                return res
            n1 = lib.ws_launch_count()
            got = {"out": out.detach()}
            res["launches"] = [n1 - n0]
            # 256 bytes fewer than the forward asked for: refused before anything is launched
            scratch.short = (len(scratch.sizes) + 1,)
            with pytest.raises(RuntimeError, match="scratch too small"):
                fused._KPBlockFn.apply(*args)
            scratch.short = ()
            if c.strided and c.kind == "resnet" and geo.inds.shape[1] <= 255:
                assert _pool_byte_record_ok(lib, c, P["feat"], c.nq) == led["arg_bytes"]
            if not c.infer:
                if c.dout_pregated:           # the consumer's decision, taken after the forward
                    lo = fused.GateLink()
                    lo.pregated, g.link_out = True, lo
                dout = b.dout.to(gpu)
                add = _dev(t["dfeat_add"], gpu)
                order = ["feat"] if c.want_dfeat else []
                order += [k for k in ("w1", "b1", "wk", "bk", "w2", "b2", "ws", "bs") if P[k] is not None]
                runs = []
                for rep in range(2):
                    if slot is not None:
                        slot.grad, slot.taken = add.clone(), False
                    hits = fused.skip_slot_hits, fused.gate_link_hits
                    n2 = lib.ws_launch_count()
                    try:
                        grads = torch.autograd.grad(out, [P[k] for k in order], dout, retain_graph=True)
                    except RuntimeError as e:
                        assert c.offset and len(str(e)) > 20, (name, str(e))
                        res["refused"] = str(e)
                        return res
                    n3 = lib.ws_launch_count()
                    runs.append(dict(zip(order, grads)))
                    assert fused.skip_slot_hits - hits[0] == (1 if c.dfeat_add else 0)
                    assert fused.gate_link_hits - hits[1] == (1 if c.gate_dfeat else 0)
                    if li is not None:
                        assert li.pregated
                res["launches"].append(n3 - n2)
                for k in order:
                    assert torch.equal(runs[0][k], runs[1][k]), (name, k)         # the same saved forward: the same bits
                for k in order:
                    got["d" + k] = runs[0][k]
                scratch.short = (len(scratch.sizes) + 1,)
                if slot is not None:
                    slot.grad, slot.taken = add.clone(), False
                with pytest.raises(RuntimeError, match="scratch too small"):
                    torch.autograd.grad(out, [P[k] for k in order], dout, retain_graph=True)
                scratch.short = ()
            torch.cuda.synchronize()
    finally:
        fused._scratch = real_scratch
        ops.clear_batch_hints()
    res["scratch_bytes"] = scratch.sizes
    assert len(scratch.sizes) == (2 if c.infer else 5), scratch.sizes
    return _judge(b, got, res)


def _run_up(gpu, name):
    from weasal_amd import fused, ops
    lib = fused._bind()
    c = B.CASES[name]
    ops.clear_batch_hints()
    b = B.build(name)
    t = b.inputs
    led = B.ledger(c)
    res = {"seed": b.seed, "tries": b.tries, "ledger": {k: str(v) for k, v in led.items()}}
    P = {k: _dev(t[k], gpu) for k in ("xc", "skip", "w", "b")}
    for v in P.values():
        if v is not None:
            v.requires_grad_(True)
    ups = b.geo.ups.to(gpu).contiguous()
    scratch, real_scratch = _Scratch(), fused._scratch
    fused._scratch = scratch
    try:
        with _Switches(c.switches):
            table = ops.col0_table(ups, c.nc)
            li = fused.GateLink() if c.gate_dxc else None
            links = [li, None]
            args = (P["xc"], P["skip"], P["w"], P["b"], ups, table, c.relu, float(c.drop), B.DROP_SEED if c.drop > 0 else 0, links)
            torch.cuda.synchronize()
            n0 = lib.ws_launch_count()
            out = fused._UpUnaryFn.apply(*args)
            n1 = lib.ws_launch_count()
            # the coarse product and the fine one, with the pool between them unless the epilogue gathers the rows itself
            assert n1 - n0 == (2 if led["forward epilogue"] == "gathered residual" else 3), (n1 - n0, led)
            scratch.short = (len(scratch.sizes) + 1,)
            with pytest.raises(RuntimeError, match="scratch too small"):
                fused._UpUnaryFn.apply(*args)
            scratch.short = ()
            if c.dout_pregated:
                lo = fused.GateLink()
                lo.pregated, links[1] = True, lo
                if c.drop > 0:
                    lo.drop = (float(c.drop), B.DROP_SEED)
            dout = b.dout.to(gpu)
            order = [k for k in ("xc", "skip", "w", "b") if P[k] is not None]
            runs = []
            for rep in range(2):
                hits = fused.gate_link_hits
                n2 = lib.ws_launch_count()
                grads = torch.autograd.grad(out, [P[k] for k in order], dout, retain_graph=True)
                n3 = lib.ws_launch_count()
                runs.append(dict(zip(order, grads)))
                assert fused.gate_link_hits - hits == (1 if c.gate_dxc else 0)
                if li is not None:
                    assert li.pregated
            res["launches"] = [n1 - n0, n3 - n2]
            for k in order:
                assert torch.equal(runs[0][k], runs[1][k]), (name, k)
            scratch.short = (len(scratch.sizes) + 1,)
            with pytest.raises(RuntimeError, match="scratch too small"):
                torch.autograd.grad(out, [P[k] for k in order], dout, retain_graph=True)
            torch.cuda.synchronize()
    finally:
        fused._scratch = real_scratch
        ops.clear_batch_hints()
    res["scratch_bytes"] = scratch.sizes
    assert len(scratch.sizes) == 5, scratch.sizes
    got = {"out": out.detach()}
    got.update({"d" + k: runs[0][k] for k in order})
    if c.drop > 0:
        keep = B.keep_mask(c).to(gpu)
        assert torch.equal(out.detach() != 0, keep) and 0.4 < float(keep.float().mean()) < 0.6       # the device hash, bit for bit
    return _judge(b, got, res)


def _judge(b, got, res):
    """ratios of every compared tensor into `res`; the failures are left to the test"""
    name = b.case.name
    if b.case.bias and b.case.unit == "kp" and b.case.ws and not b.case.infer:
        assert torch.equal(got["dbs"], got["db2"])                      # fused.py hands the shortcut bias a copy of db2
    res["ratios"], res["bad"] = {}, []
    for k, (err, bd, ratio) in B.ratios(b, got).items():
        finite = bool(torch.isfinite(got[k]).all())
        print("%-30s seed %4d %-6s |dev - ref64| %.3e  float32 on the CPU %.3e  bound %.3e  ratio %.3f  max|ref| %.3e" % (
            name, b.seed, k, err, b.err32[k], bd, ratio, float(b.ref64[k].abs().max())))
        res["ratios"][k] = {"err": err, "err32": b.err32[k], "bound": bd, "ratio": ratio if finite else float("inf")}
        if not finite or not err <= bd:
            res["bad"].append((k, err, bd))
    return res


def _result(gpu, name):
    if name not in _RESULTS:
        try:
            _RESULTS[name] = (_run_kp if B.CASES[name].unit == "kp" else _run_up)(gpu, name)
        finally:
            _dump()
    return _RESULTS[name]


@pytest.mark.parametrize("name", [c.name for c in B.KP_CASES])
def test_kpblock_branch_vs_float64(gpu, name):
    res = _result(gpu, name)
    if "refused" in res:                                                # only a misaligned case may say no, and says why
        assert B.CASES[name].offset, res
        return
    assert not res["bad"], (name, res["bad"])


@pytest.mark.parametrize("name", [c.name for c in B.UP_CASES])
def test_upunary_branch_vs_float64(gpu, name):
    res = _result(gpu, name)
    assert not res["bad"], (name, res["bad"])


def test_grouping_and_fusing_change_the_launch_counts(gpu):
    """observed, not assumed: where the ledger says pair_in / grouped the leaf products share their launches, and unary1 +
    shortcut projection ride in one launch when they share an instantiation (equal widths; at 64 -> 32 beside 64 -> 128 the
    group is two launches of one member each), against ws_block_group_rows = 0 on the same shapes; the forward-only 32 -> 32
    layer is one launch fewer than gather + product"""
    base, single = _result(gpu, "resnet_64_128"), _result(gpu, "switch_group_rows_0")
    assert base["rows"][:2] == single["rows"][:2]
    assert base["launches"][0] <= single["launches"][0], (base["launches"], single["launches"])
    assert base["launches"][1] < single["launches"][1], (base["launches"], single["launches"])
    base, single = _result(gpu, "resnet_64_32_32"), _result(gpu, "switch_group_rows_0_64_32_32")
    assert base["launches"][0] == single["launches"][0] - 1, (base["launches"], single["launches"])
    assert base["launches"][1] < single["launches"][1], (base["launches"], single["launches"])
    up, up_single = _result(gpu, "up_relu"), _result(gpu, "up_switch_group_rows_0")
    assert up["launches"][1] == up_single["launches"][1] - 2, (up["launches"], up_single["launches"])
    one, two = _result(gpu, "infer_one_launch"), _result(gpu, "infer_two_launches")
    assert one["launches"][0] == two["launches"][0] - 1, (one["launches"], two["launches"])


def test_table_walk_takes_the_packed_kernel_on_the_strided_shapes(gpu):
    """the strided cases really reach the packed K4 (the reporter of ws_kpconv_gather_bwd_x_packed), the self-query ones
    what the gated entry launches"""
    from weasal_amd import fused
    lib = fused._bind()
    buf = C.create_string_buffer(200)
    a = torch.empty(64, device=gpu)
    for name, packed in (("strided_projection", True), ("strided_feat_offset_add", True), ("resnet_64_128", False)):
        c = B.CASES[name]
        h = B.build(name).geo.inds.shape[1]
        assert lib.ws_kpconv_gather_bwd_x_packed_variant(c.nq, c.ns, h, c.conv_in, C.c_void_p(a.data_ptr()), C.c_void_p(a.data_ptr()), 0, 0, 0, 0,
                                                         0, 1 if c.orders else 0, buf, 200) == 0
        assert (buf.value != b"none") == packed, (name, buf.value)
