"""GPU: the block calls (ws_kpblock_fwd / ws_kpblock_bwd / ws_upunary_bwd, weasal_amd/csrc/blocks.hip) with their independent
dense products grouped (ws_block_group_rows at its default) against the single launches in their old order (0).

Grouping changes how many launches a call makes and when the leaf products run, never a plan and never the order of a sum:
every output and every gradient buffer must be BIT-identical.  The launch count (ws_launch_count) must fall, and the
scratch-size queries must cover the run: every call here runs with exactly the queried bytes, and 256 fewer are refused
(WS_ERR_CAPACITY)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _switch():
    from weasal_amd import fused
    return C.c_int64.in_dll(fused._bind(), "ws_block_group_rows")


def _geometry(gpu, ns, nq, radius, seed):
    """s_pts [ns, 3] in a box of ~25 neighbours per ball, q_pts = every (ns // nq)-th support; (batch, slot)"""
    from weasal_amd import fused, ops
    g = torch.Generator().manual_seed(seed)
    side = radius * (ns * 4.19 / 25.0) ** (1.0 / 3.0)
    s = (torch.rand(ns, 3, generator=g) * side).to(gpu)
    lens_s = np.array([ns - ns // 3, ns // 3], np.int32)
    if nq == ns:
        q, lens_q = s, lens_s
    else:
        step = ns // nq
        q = s[::step][:nq].contiguous()
        first = int(torch.arange(ns)[::step][:nq].lt(int(lens_s[0])).sum())
        lens_q = np.array([first, nq - first], np.int32)
    neigh = ops.radius_neighbors(s, s, lens_s, lens_s, radius, dtype=torch.int64)
    pools = ops.radius_neighbors(q, s, lens_q, lens_s, radius, dtype=torch.int64)
    slot = fused.SkipSlot()
    return types.SimpleNamespace(points=[s, q], neighbors=[neigh], pools=[pools], skip_slot=None), slot


def _cfg(use_bn):
    from weasal_amd import config as wcfg
    cfg = wcfg.DALESPLConfig()
    cfg.use_batch_norm = use_bn
    return cfg


def _run(lib, fwd_bwd, value):
    """(tensors, launches forward, launches backward) of one forward + backward with the switch at `value`"""
    sw = _switch()
    old = sw.value
    sw.value = value
    try:
        return fwd_bwd(lib)
    finally:
        sw.value = old


def _kp_case(gpu, name, in_dim, out_dim, ns, nq, use_bn, add=False, seed=5):
    from weasal_amd import blocks
    radius = 0.5
    batch, slot = _geometry(gpu, ns, nq, radius, seed)
    torch.manual_seed(seed)
    np.random.seed(seed)
    cfg = _cfg(use_bn)
    cls = blocks.SimpleBlock if name.startswith("simple") else blocks.ResnetBottleneckBlock
    blk = cls(name, in_dim, out_dim, radius, 0, cfg).to(gpu).train()
    with torch.no_grad():
        for n_, p in blk.named_parameters():
            if n_.endswith(".bias"):
                p.normal_(0.0, 0.1)
    x = torch.randn(ns, in_dim, device=gpu)
    n_out = out_dim // 2 if name.startswith("simple") else out_dim
    dy = torch.randn(nq, n_out, device=gpu)
    extra = torch.randn(ns, in_dim, device=gpu) if add else None
    if add:
        batch.skip_slot = slot

    def fwd_bwd(lib):
        xr = x.clone().requires_grad_(True)
        blk.zero_grad(set_to_none=True)
        slot.grad, slot.armed, slot.taken = None, False, False
        c0 = lib.ws_launch_count()
        out = blk(xr, batch)
        c1 = lib.ws_launch_count()
        if add:
            assert slot.armed
            slot.grad = extra.clone()
        out.backward(dy)
        c2 = lib.ws_launch_count()
        torch.cuda.synchronize()
        t = {"out": out.detach().clone(), "dx": xr.grad.clone()}
        for n_, p in blk.named_parameters():
            if p.grad is not None:
                t["d_" + n_] = p.grad.clone()
        return t, c1 - c0, c2 - c1
    return fwd_bwd


KP_CASES = {
    # the issue's shapes: resnet block with projection, in 64, conv 32 -> 32, out 128, nq = ns = 700
    "resnet_projection": dict(name="resnetb", in_dim=64, out_dim=128, ns=700, nq=700),
    # wide enough that the pairs share an instantiation: unary1 + shortcut in the forward, dscin + g2 (both split-K) in the backward
    "resnet_projection_wide": dict(name="resnetb", in_dim=256, out_dim=512, ns=700, nq=700),
    "resnet_identity_shortcut": dict(name="resnetb", in_dim=128, out_dim=128, ns=700, nq=700),
    "resnet_strided_dfeat_add": dict(name="resnetb_strided", in_dim=64, out_dim=128, ns=700, nq=233, add=True),
    "simple": dict(name="simple", in_dim=64, out_dim=128, ns=700, nq=700),
}


@pytest.mark.parametrize("use_bn", [True, False])
@pytest.mark.parametrize("case", sorted(KP_CASES))
def test_kpblock_grouped_is_bit_identical_and_launches_less(gpu, case, use_bn):
    """use_bn False: the BatchNormBlock biases and their gradients are live (no gated epilogues)"""
    from weasal_amd import fused
    lib = fused._bind()
    default = _switch().value
    assert default > 700, "the default row limit must take these blocks"
    fwd_bwd = _kp_case(gpu, use_bn=use_bn, **KP_CASES[case])
    _run(lib, fwd_bwd, 0)                          # (builds the transposed tables: their launches are not the block's)
    t1, f1, b1 = _run(lib, fwd_bwd, default)
    t0, f0, b0 = _run(lib, fwd_bwd, 0)
    assert t1.keys() == t0.keys() and len(t1) >= 3
    for k in t0:
        assert torch.equal(t1[k], t0[k]), k
        assert bool(torch.isfinite(t0[k]).all()), k
    assert f1 <= f0 and b1 <= b0, (f1, f0, b1, b0)
    if case != "simple":                           # (a simple block has one weight-gradient product: nothing to share)
        assert b1 < b0, (b1, b0)                   # the collected weight-gradient products share launches
    if case == "resnet_projection_wide":
        assert f1 == f0 - 1, (f1, f0)              # unary1 + shortcut projection: one launch
        # 4 dW products + 4 reductions -> 1 + 1; dscin + g2 with their split epilogues: 4 kernels -> 2 (counted 2 -> 2: a
        # single split product and its epilogue pass the launch check together)
        assert b1 == b0 - 6, (b1, b0)


def test_upunary_grouped_is_bit_identical_and_launches_less(gpu):
    from weasal_amd import fused
    from weasal_amd.blocks import UnaryBlock
    lib = fused._bind()
    default = _switch().value
    nc, nf, c_up, c_skip, out_dim = 300, 700, 128, 128, 64
    torch.manual_seed(3)
    unary = UnaryBlock(c_up + c_skip, out_dim, False, 0).to(gpu)
    with torch.no_grad():
        unary.batch_norm.bias.normal_()
    x = torch.randn(nc, c_up, device=gpu)
    skip = torch.randn(nf, c_skip, device=gpu)
    ups = torch.randint(0, nc, (nf, 3), device=gpu)
    ups[::17, 0] = nc
    dy = torch.randn(nf, out_dim, device=gpu)

    def fwd_bwd(lib):
        xr, sr = x.clone().requires_grad_(True), skip.clone().requires_grad_(True)
        unary.zero_grad(set_to_none=True)
        c0 = lib.ws_launch_count()
        out = fused.upunary(xr, sr, unary, ups)
        c1 = lib.ws_launch_count()
        out.backward(dy)
        c2 = lib.ws_launch_count()
        torch.cuda.synchronize()
        t = {"out": out.detach().clone(), "dx": xr.grad.clone(), "dskip": sr.grad.clone()}
        for n_, p in unary.named_parameters():
            if p.grad is not None:
                t["d_" + n_] = p.grad.clone()
        return t, c1 - c0, c2 - c1
    _run(lib, fwd_bwd, 0)                          # (builds the upsampling table)
    t1, f1, b1 = _run(lib, fwd_bwd, default)
    t0, f0, b0 = _run(lib, fwd_bwd, 0)
    assert "d_mlp.weight" in t0
    for k in t0:
        assert torch.equal(t1[k], t0[k]), k
    assert f1 == f0 and b1 == b0 - 2, (f1, f0, b1, b0)         # two pitched products + two reductions -> 1 + 1


@pytest.mark.parametrize("value", [None, 0])
def test_scratch_queries_cover_the_run_and_less_is_refused(gpu, monkeypatch, value):
    """the calls above run with exactly the queried bytes (fused._scratch); 256 fewer: WS_ERR_CAPACITY, forward and backward"""
    from weasal_amd import fused
    lib = fused._bind()
    value = _switch().value if value is None else value
    fwd_bwd = _kp_case(gpu, use_bn=True, **KP_CASES["resnet_projection_wide"])
    real = fused._scratch
    seen = []

    def exact(nbytes, device):
        seen.append(int(nbytes))
        return real(nbytes, device)
    monkeypatch.setattr(fused, "_scratch", exact)
    _run(lib, fwd_bwd, value)
    assert len(seen) == 2 and all(n >= 256 and n % 256 == 0 for n in seen), seen      # (so _scratch did not round them up)
    monkeypatch.setattr(fused, "_scratch", lambda nbytes, device: real(int(nbytes) - 256, device))
    with pytest.raises(RuntimeError, match="scratch too small"):
        _run(lib, fwd_bwd, value)
    # the backward alone: forward with the real size, then the short one
    calls = {"n": 0}

    def short_second(nbytes, device):
        calls["n"] += 1
        return real(int(nbytes) - (256 if calls["n"] == 2 else 0), device)
    monkeypatch.setattr(fused, "_scratch", short_second)
    with pytest.raises(RuntimeError, match="scratch too small"):
        _run(lib, fwd_bwd, value)
    assert calls["n"] == 2


def test_empty_blocks(gpu):
    """nq = ns = 0 and an empty decoder step: every gradient buffer is cleared, with grouping on and off alike"""
    from weasal_amd import fused
    lib = fused._bind()
    default = _switch().value
    dummy = torch.zeros(4096, device=gpu)
    res = {}
    for value in (default, 0):
        sw = _switch()
        sw.value = value
        try:
            d = fused.KPBlockDesc()
            for f in ("q_pts", "s_pts", "inds", "kernel_points", "feat", "wk", "wf", "out", "w1", "w2", "ws", "x1", "x2", "dout"):
                setattr(d, f, dummy.data_ptr())
            d.nq = d.ns = 0
            d.h, d.k, d.extent, d.slope = 3, 15, 1.0, 0.1
            d.in_dim, d.conv_in, d.conv_out, d.out_dim = 64, 32, 32, 128
            grads = {"dw1": 32 * 64, "dwk": 15 * 32 * 32, "dw2": 128 * 32, "dws": 128 * 64, "db1": 32, "dbk": 32, "db2": 128}
            bufs = {k: torch.full((n,), float("nan"), device=gpu) for k, n in grads.items()}
            for k, t in bufs.items():
                setattr(d, k, t.data_ptr())
            nb = lib.ws_kpblock_bwd_scratch_bytes(C.byref(d))
            assert nb >= 256 and nb % 256 == 0
            scr = torch.empty(nb, dtype=torch.uint8, device=gpu)
            assert lib.ws_kpblock_bwd(C.byref(d), scr.data_ptr(), nb, None) == 0, lib.ws_last_error()
            assert lib.ws_kpblock_bwd(C.byref(d), scr.data_ptr(), nb - 256, None) == 5
            nf_ = lib.ws_kpblock_fwd_scratch_bytes(C.byref(d))
            assert lib.ws_kpblock_fwd(C.byref(d), scr.data_ptr() if nf_ <= nb else torch.empty(nf_, dtype=torch.uint8, device=gpu).data_ptr(),
                                      nf_, None) == 0, lib.ws_last_error()
            u = fused.UpUnaryDesc()
            for f in ("xc", "skip", "ups", "w", "out", "yc", "dout", "dxc", "dskip", "t_offsets", "t_pairs"):
                setattr(u, f, dummy.data_ptr())
            u.nc = u.nf = 0
            u.c_up, u.c_skip, u.out_dim, u.ldw, u.h_up, u.relu, u.slope = 64, 32, 32, 96, 1, 1, 0.1
            dw = torch.full((32 * 96,), float("nan"), device=gpu)
            db = torch.full((32,), float("nan"), device=gpu)
            u.dw, u.db = dw.data_ptr(), db.data_ptr()
            nu = lib.ws_upunary_bwd_scratch_bytes(C.byref(u))
            su = torch.empty(nu, dtype=torch.uint8, device=gpu)
            assert lib.ws_upunary_bwd(C.byref(u), su.data_ptr(), nu, None) == 0, lib.ws_last_error()
            torch.cuda.synchronize()
            res[value] = dict(bufs, dw=dw, db=db)
        finally:
            sw.value = default
    for k in res[0]:
        assert bool((res[0][k] == 0).all()) and torch.equal(res[0][k], res[default][k]), k


def test_rows_on_one_side_only_are_refused(gpu):
    """supports without queries / coarse rows without fine rows are the empty calls above; the other way round the forward
    is act(bias) rows (kpblock: ns = 0, nq > 0) or act(skip @ Ws^T + b) (upunary: nc = 0, nf > 0) with live bias, weight and
    skip gradients, which a zero-gradient exit would contradict.  No caller sends either: both entries and both scratch
    queries say WS_ERR_UNSUPPORTED and name the sizes"""
    from weasal_amd import fused
    lib = fused._bind()
    dummy = torch.zeros(4096, device=gpu)
    scr = torch.empty(1 << 20, dtype=torch.uint8, device=gpu)
    d = fused.KPBlockDesc()
    for f in ("q_pts", "s_pts", "inds", "kernel_points", "feat", "wk", "wf", "out", "w1", "w2", "ws", "x1", "x2", "dout", "pooled", "arg",
              "dw1", "dwk", "dw2", "dws", "t_offsets", "t_pairs"):
        setattr(d, f, dummy.data_ptr())
    d.nq, d.ns, d.strided = 5, 0, 1
    d.h, d.k, d.extent, d.slope = 3, 15, 1.0, 0.1
    d.in_dim, d.conv_in, d.conv_out, d.out_dim = 64, 32, 32, 128
    for query in (lib.ws_kpblock_fwd_scratch_bytes, lib.ws_kpblock_bwd_scratch_bytes):
        assert query(C.byref(d)) == -1 and b"nq=5 ns=0" in lib.ws_last_error()
    for call in (lib.ws_kpblock_fwd, lib.ws_kpblock_bwd):
        assert call(C.byref(d), scr.data_ptr(), scr.numel(), None) == 2 and b"nq=5 ns=0" in lib.ws_last_error()
    d.nq, d.ns = 0, 5                                # supports without queries stay an empty call: zero gradients
    assert lib.ws_kpblock_bwd_scratch_bytes(C.byref(d)) >= 256
    u = fused.UpUnaryDesc()
    for f in ("xc", "skip", "ups", "w", "out", "yc", "dout", "dxc", "dskip", "t_offsets", "t_pairs", "dw"):
        setattr(u, f, dummy.data_ptr())
    u.nc, u.nf = 0, 7
    u.c_up, u.c_skip, u.out_dim, u.ldw, u.h_up, u.relu, u.slope = 64, 32, 32, 96, 1, 1, 0.1
    for query in (lib.ws_upunary_fwd_scratch_bytes, lib.ws_upunary_bwd_scratch_bytes):
        assert query(C.byref(u)) == -1 and b"nc=0 nf=7" in lib.ws_last_error()
    for call in (lib.ws_upunary_fwd, lib.ws_upunary_bwd):
        assert call(C.byref(u), scr.data_ptr(), scr.numel(), None) == 2 and b"nc=0 nf=7" in lib.ws_last_error()
    u.nc, u.nf = 7, 0
    assert lib.ws_upunary_bwd_scratch_bytes(C.byref(u)) >= 256
    torch.cuda.synchronize()
