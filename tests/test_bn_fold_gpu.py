"""GPU: evaluation-mode batch normalisation folded into the products (weasal_amd/csrc/bn_fold.hip, ops.bn_fold, the blocks
and networks that use it) against tests/bn_fold_ref.py and the CPU network in float64.

1. / 2. The C entries are called directly (ctypes) on the test's own buffers, row by row of bn_fold_ref.ROWS: every output is
   NaN in its live region before the call, every buffer carries guard rows holding a finite sentinel that must come back
   bit-unchanged, and every call runs twice into fresh buffers (torch.equal).  The bounds count roundings and are stated in
   bn_fold_ref (w_out, dw: 4 * 2^-23 relative; t_out: 5 * 2^-23 (|beta| + |mean a|); dgamma: the worst case of a float32
   sum of its length; dbeta: the bits of dt_out).  A table of WS_BN_FOLD_MAX + 1 sites makes the launcher loop.
3. ops.bn_fold gives the bits of the raw calls on a three-site list one of whose sites requires no gradient.
4. Blocks, 5. networks, 7. no stale weights: the folded route against the same modules on the CPU in float64 under
   oracle.kpconv_ref.cpu_reference_mode, per tensor

       max |folded - ref64|  <=  4 * max |fold-off route - ref64|  +  1e-6 * max |ref64|

   and the fused routes were taken: the library launches of the folded module, the fold's own counted apart, equal those
   of the same module in reference mode.
6. Frozen statistics with gradients: BatchNorm1d modules in eval() inside a training step reach the fused training routes.
8. Reference mode and 'points' in training mode do not see the switch: same bits with WEASAL_BN_FOLD unset and 0 (a fresh
   child process, which also gives test 5 the parent commit's evaluation route).

Every comparison prints its figures before it asserts.

Worst figures on the MI355X.  Raw calls, error in units of 2^-23 |ref| (2^-23 (|beta| + |mean a|) for t_out), bounds 4 / 4 / 5:
w_out 1.54, dw 1.63, t_out 1.47; dgamma 1.03 of 2^-24 sum |terms| + 2^-23 |ref| where the bound allows (L + 8) and 4 of the
two.  Folded error over the fold-off route's error against the CPU in float64, bound 4: blocks 1.105 (resnetb-projected),
KPFCNN logits 1.124, KPFCNN_mprm 1.690 (a class-activation map: 7.2e-8 against 4.2e-8), the forward after a training step
0.896.  Frozen statistics: logits 9.3e-8, worst gradient 1.2e-6 (encoder_blocks.2.KPConv.weights) relative to the CPU step.
"""
import copy
import ctypes as C
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import bn_fold_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                      # guard floats on either side of every buffer
SENTINEL = 12345.678
_BITS = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32).item()


def _L():
    from weasal_amd import _lib
    return _lib


class Guarded:
    """`numel` live floats on the device between two runs of GUARD sentinel floats, `offset` floats (4 bytes each) off the
    16-byte alignment of the allocation: the live part holds `src` or NaN"""

    def __init__(self, gpu, numel, src=None, offset=0):
        lead = GUARD + offset                     # GUARD is a multiple of 4: the live part is `offset` floats off 16 bytes
        self.flat = torch.full((lead + numel + GUARD,), SENTINEL, dtype=torch.float32, device=gpu)
        self.live = self.flat[lead:lead + numel]
        assert self.flat.data_ptr() % 16 == 0 and self.live.data_ptr() % 16 == 4 * (offset % 4)
        if src is None:
            self.live.fill_(float("nan"))
        else:
            self.live.copy_(src.reshape(-1).to(gpu))
        self.lead, self.numel = lead, numel

    @property
    def ptr(self):
        return self.live.data_ptr()

    def value(self):
        return self.live.clone()

    def intact(self):
        rest = torch.cat((self.flat[:self.lead], self.flat[self.lead + self.numel:]))
        return bool((rest.view(torch.int32) == _BITS).all())


def _arr(kind, values):
    if kind is None:
        return (C.c_void_p * len(values))(*[None if v is None else v.ptr for v in values])
    return (kind * len(values))(*values)


def raw(gpu, sites, tag, launches=1):
    """ws_bn_fold_fwd + ws_bn_fold_bwd of a table [(row, inputs)] on guarded, poisoned buffers -> [{tensor: value}]"""
    L = _L()
    lib = L.lib()
    st = L.current_stream()
    n = len(sites)
    bufs = []
    for row, ins in sites:
        numel = row["outer"] * row["c"] * row["inner"]
        so, do = (1 if row["off"] == "src" else 0), (1 if row["off"] == "dst" else 0)
        b = {"w": Guarded(gpu, numel, ins["w"], so), "w_out": Guarded(gpu, numel, None, do), "t_out": Guarded(gpu, row["c"])}
        for k in ("gamma", "beta", "mean", "var"):
            b[k] = Guarded(gpu, row["c"], ins[k], 1)                       # [c] vectors: any alignment
        b["dw_out"] = Guarded(gpu, numel, ins["dw_out"], so) if ins["dw_out"] is not None else None
        b["dt_out"] = Guarded(gpu, row["c"], ins["dt_out"]) if ins["dt_out"] is not None else None
        b["dw"], b["dgamma"], b["dbeta"] = Guarded(gpu, numel, None, do), Guarded(gpu, row["c"]), Guarded(gpu, row["c"])
        bufs.append(b)
    col = lambda k: _arr(None, [b[k] for b in bufs])
    outer, c, inner = (_arr(t, [row[k] for row, _ in sites]) for t, k in ((C.c_int64, "outer"), (C.c_int32, "c"), (C.c_int64, "inner")))
    eps = _arr(C.c_float, [R.EPS] * n)
    before = lib.ws_launch_count()
    L.check(lib.ws_bn_fold_fwd(col("w"), outer, c, inner, col("gamma"), col("beta"), col("mean"), col("var"), eps, col("w_out"),
                               col("t_out"), n, st))
    torch.cuda.synchronize()
    assert lib.ws_launch_count() - before == launches, tag
    before = lib.ws_launch_count()
    L.check(lib.ws_bn_fold_bwd(col("w"), outer, c, inner, col("gamma"), col("mean"), col("var"), eps, col("dw_out"), col("dt_out"),
                               col("dw"), col("dgamma"), col("dbeta"), n, st))
    torch.cuda.synchronize()
    assert lib.ws_launch_count() - before == launches, tag
    out = []
    for (row, _), b in zip(sites, bufs):
        for name, g in b.items():
            assert g is None or g.intact(), "%s %s: guard of %s overwritten" % (tag, row["id"], name)
        res = {k: b[k].value() for k in ("w_out", "t_out", "dw", "dgamma", "dbeta")}
        for name, v in res.items():
            assert bool(torch.isfinite(v).all()), "%s %s: %s has non-finite elements (a missed store?)" % (tag, row["id"], name)
        out.append(res)
    return out


def _report(tag, got, ref, ins):
    """print each tensor's error in units of its bound's scale, then assert the bounds"""
    unit = {"w_out": R.ULP * ref["w_out"].abs(), "dw": R.ULP * ref["dw"].abs(),
            "t_out": R.ULP * (ins["beta"].double().abs() + (ins["mean"].double() * ref["a"]).abs()),
            "dgamma": 2.0 ** -24 * ref["dgamma_abs"] + R.ULP * ref["dgamma"].abs()}
    line = []
    for k, u in unit.items():
        err = (got[k].double().cpu().reshape(ref[k].shape) - ref[k]).abs()
        line.append("%s %.2f" % (k, float((err / u.clamp(min=1e-300)).max()) if err.numel() else 0.0))
    print("site %-34s error / (2^-23 scale; dgamma: 2^-24 sum|terms| + 2^-23 |ref|): %s" % (tag, "  ".join(line)))
    bad = R.violations(got, ref, ins)
    assert not bad, (tag, bad)


@pytest.mark.parametrize("row_id", [r["id"] for r in R.ROWS])
def test_fold_branch(gpu, row_id):
    row = R.BY_ID[row_id]
    ins, ref = R.case(row_id)
    first = raw(gpu, [(row, ins)], row_id)[0]
    _report(row_id, first, ref, ins)
    again = raw(gpu, [(row, ins)], row_id + " again")[0]
    for key, v in first.items():
        assert torch.equal(v, again[key]), "%s: %s differs run to run" % (row_id, key)


def test_table_longer_than_a_launch(gpu):
    """WS_BN_FOLD_MAX + 1 sites of mixed shapes: two launches each way, every site held as if it were alone"""
    ids = ["linear-c130-k129", "kpconv-K15-ci32-co66", "linear-c3-k1", "kpconv-K15-ci80-co32-tall", "linear-c32-k32-src-off",
           "kpconv-K9-ci1-co4", "linear-c130-k2052-chunks", "mid-o3-c5-i7", "kpconv-K15-ci4-co32-no-dw", "linear-c32-k32-no-dt",
           "linear-c1-k1"]
    sites = []
    for i in range(R.WS_BN_FOLD_MAX + 1):
        row = R.BY_ID[ids[i % len(ids)]]
        sites.append((row, R.inputs(row, seed=5000 + i)))
    first = raw(gpu, sites, "table", launches=2)
    for (row, ins), got in zip(sites, first):
        _report("table/" + row["id"], got, R.reference(ins), ins)
    again = raw(gpu, sites, "table again", launches=2)
    assert all(torch.equal(a[k], b[k]) for a, b in zip(first, again) for k in a)
    # sites without channels are passed over; nothing but such sites launches nothing
    L = _L()
    lib = L.lib()
    z = _arr(None, [None, None])
    before = lib.ws_launch_count()
    L.check(lib.ws_bn_fold_fwd(z, _arr(C.c_int64, [1, 1]), _arr(C.c_int32, [0, 0]), _arr(C.c_int64, [4, 4]), z, z, z, z,
                               _arr(C.c_float, [R.EPS] * 2), z, z, 2, L.current_stream()))
    assert lib.ws_launch_count() == before


# ------------------------------------------------------------------------------------------------------------------
# 3. the operator
# ------------------------------------------------------------------------------------------------------------------
def _bn_module(gpu, ins, grad=True):
    c = ins["gamma"].shape[0]
    bn = torch.nn.BatchNorm1d(c, eps=R.EPS)
    with torch.no_grad():
        bn.weight.copy_(ins["gamma"]), bn.bias.copy_(ins["beta"]), bn.running_mean.copy_(ins["mean"]), bn.running_var.copy_(ins["var"])
    bn = bn.to(gpu).eval()
    bn.weight.requires_grad_(grad), bn.bias.requires_grad_(grad)
    return bn


def test_ops_path_gives_the_bits_of_the_raw_calls(gpu):
    from weasal_amd import ops
    shapes = {"linear-c32-k32": (32, 32), "kpconv-K15-ci4-co32": (15, 4, 32), "linear-c130-k129": (130, 129)}
    axes = {"linear-c32-k32": 0, "kpconv-K15-ci4-co32": 2, "linear-c130-k129": 0}
    frozen = "kpconv-K15-ci4-co32"                                       # this site requires no gradient
    sites = [(R.BY_ID[k], R.case(k)[0]) for k in shapes]
    want = raw(gpu, sites, "ops")
    ws, bns = {}, {}
    for k, (row, ins) in zip(shapes, sites):
        ws[k] = ins["w"].reshape(shapes[k]).to(gpu).requires_grad_(k != frozen)
        bns[k] = _bn_module(gpu, ins, grad=k != frozen)
    lib = _L().lib()
    before, counted = lib.ws_launch_count(), ops.bn_fold_launches
    pairs = ops.bn_fold([(ws[k], axes[k], bns[k]) for k in shapes])
    assert lib.ws_launch_count() - before == 1 and ops.bn_fold_launches - counted == 1
    loss = 0
    for k, (row, ins), (wf, t), w_ in zip(shapes, sites, pairs, want):
        assert wf.shape == ws[k].shape and torch.equal(wf.detach().reshape(-1), w_["w_out"]) and torch.equal(t.detach(), w_["t_out"]), k
        loss = loss + (wf * ins["dw_out"].reshape(shapes[k]).to(gpu)).sum() + (t * ins["dt_out"].to(gpu)).sum()
    before = lib.ws_launch_count()
    loss.backward()
    assert lib.ws_launch_count() - before == 1 and ops.bn_fold_launches - counted == 2
    for k, (row, ins), w_ in zip(shapes, sites, want):
        bn = bns[k]
        if k == frozen:
            assert ws[k].grad is None and bn.weight.grad is None and bn.bias.grad is None
            continue
        got = {"dw": ws[k].grad.reshape(-1), "dgamma": bn.weight.grad, "dbeta": bn.bias.grad}
        for name, v in got.items():
            assert torch.equal(v, w_[name]), "%s: %s differs from the raw call" % (k, name)
        _report("ops/" + k, {**got, "w_out": w_["w_out"], "t_out": w_["t_out"]}, R.case(k)[1], ins)
        assert bn.running_mean.grad is None and bn.running_var.grad is None
    # a folded weight used without its bias: the bias gradient is NULL, dbeta zeros
    k = "linear-c32-k32"
    ws[k].grad = bns[k].weight.grad = bns[k].bias.grad = None
    (wf, t), = ops.bn_fold([(ws[k], 0, bns[k])])
    wf.square().sum().backward()
    assert not bns[k].bias.grad.any() and ws[k].grad.abs().sum() > 0
    with pytest.raises(ValueError):
        ops.bn_fold([(ws[k].detach().to(torch.bfloat16), 0, bns[k])])
    with pytest.raises(ValueError):
        ops.bn_fold([(ws[k], 1, _bn_module(gpu, R.case("linear-c3-k1")[0]))])


# ------------------------------------------------------------------------------------------------------------------
# modules: helpers
# ------------------------------------------------------------------------------------------------------------------
import test_batchnorm_gpu as T                 # _net_config, _golden_batch, _make_net: the architecture of the existing test


def _move_bn(module, seed=3):
    """BN parameters and buffers off their initial 1 / 0 (as T._make_net does), so that a swap would show"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in list(module.named_parameters()) + list(module.named_buffers()):
            if name.endswith("batch_norm.weight"):
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
            elif name.endswith("batch_norm.bias") or name.endswith("running_mean"):
                t.copy_(torch.randn(t.shape, generator=g) * 0.1)
            elif name.endswith("running_var"):
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
    return module


def _batch64(batch, extra=()):
    from weasal_amd.pyramid import PyramidBatch
    cast = lambda t: t.detach().cpu().double() if t.is_floating_point() else t.detach().cpu()
    flat = batch.points + batch.neighbors + batch.pools + batch.upsamples + batch.lengths + [batch.features, batch.labels]
    b = PyramidBatch([cast(t) for t in flat])
    for name in extra:
        setattr(b, name, cast(getattr(batch, name)))
    return b


def _copy64(fresh, net):
    """the state of `net` in a fresh CPU module in float64 (a trained module holds its last loss: no deepcopy)"""
    fresh.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
    return fresh.double().eval()


class _fold_switch:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from weasal_amd import ops
        self.old, ops.BN_FOLD = ops.BN_FOLD, self.on

    def __exit__(self, *exc):
        from weasal_amd import ops
        ops.BN_FOLD = self.old


def _counted(fn):
    """(result, library launches without the fold's, the fold's launches)"""
    from weasal_amd import ops
    lib = _L().lib()
    torch.cuda.synchronize()
    a, f = lib.ws_launch_count(), ops.bn_fold_launches
    out = fn()
    torch.cuda.synchronize()
    folds = ops.bn_fold_launches - f
    return out, lib.ws_launch_count() - a - folds, folds


_RATIOS = {}


def _held(tag, folded, off, ref64):
    tensors = lambda v: list(v) if isinstance(v, (tuple, list)) else [v]
    flat = lambda v: [t for x in tensors(v) for t in tensors(x)]
    for i, (a, b, r) in enumerate(zip(flat(folded), flat(off), flat(ref64))):
        r = r.detach().double().cpu()
        ef, eo = float((a.detach().double().cpu() - r).abs().max()), float((b.detach().double().cpu() - r).abs().max())
        bound = 4 * eo + 1e-6 * float(r.abs().max())
        _RATIOS["%s[%d]" % (tag, i)] = ef / eo if eo else 0.0
        print("%-44s tensor %d  folded %.3e  fold-off %.3e  ratio %.3f  max|ref| %.3e" % (tag, i, ef, eo, ef / eo if eo else 0.0, float(r.abs().max())))
        assert ef <= bound, (tag, i, ef, eo)


def _block_cases(gpu):
    """name -> (make(mode) -> module, call(module, batch, inputs) -> output, input shapes, fold sites)"""
    from weasal_amd.architectures import KPFCNN
    from weasal_amd.blocks import NearestUpsampleBlock, ResnetBottleneckBlock, SimpleBlock, SimpleBlock2, UnaryBlock
    base = T._net_config('points')
    radius = lambda layer: base.first_subsampling_dl * base.conv_radius * 2 ** layer

    def cfg(mode):
        return T._net_config(mode)

    def unary(no_relu):
        return lambda mode: UnaryBlock(32, 64, True, 0.02, no_relu=no_relu, bn_mode=mode)

    def block(cls, name, i, o, layer):
        return lambda mode: cls(name, i, o, radius(layer), layer, cfg(mode))
    rows = {1: 1607, 2: 341}
    plain = lambda m, b, x: m(x[0], b)
    cases = {}
    for no_relu in (False, True):
        for res in (False, True):
            cases["unary%s%s" % ("-norelu" if no_relu else "", "-res" if res else "")] = (
                unary(no_relu), (lambda m, b, x: m.forward_fused(x[0], residual=x[1], batch=b)) if res else (lambda m, b, x: m(x[0], b)),
                [(rows[2], 32), (rows[2], 64)] if res else [(rows[2], 32)], 1)
    cases["simple"] = (block(SimpleBlock, "simple", 32, 64, 2), plain, [(rows[2], 32)], 1)
    cases["simple2"] = (block(SimpleBlock2, "simple", 32, 32, 2), plain, [(rows[2], 32)], 1)
    cases["resnetb-projected"] = (block(ResnetBottleneckBlock, "resnetb", 32, 64, 2), plain, [(rows[2], 32)], 4)
    cases["resnetb-identity-shortcut"] = (block(ResnetBottleneckBlock, "resnetb", 64, 64, 2), plain, [(rows[2], 64)], 3)
    cases["resnetb-identity-unary1"] = (block(ResnetBottleneckBlock, "resnetb", 16, 64, 2), plain, [(rows[2], 16)], 3)
    cases["resnetb-strided-projected"] = (block(ResnetBottleneckBlock, "resnetb_strided", 32, 64, 1), plain, [(rows[1], 32)], 4)
    cases["resnetb-strided-identity-shortcut"] = (block(ResnetBottleneckBlock, "resnetb_strided", 64, 64, 1), plain, [(rows[1], 64)], 3)

    def step(m, b, x):
        return KPFCNN._fused_upsample_unary(None, x[0], x[1], NearestUpsampleBlock(2), m, b)
    cases["decoder-step"] = (lambda mode: UnaryBlock(96, 32, True, 0.02, bn_mode=mode), step, [(rows[2], 64), (rows[1], 32)], 1)
    return cases


_BLOCKS = ["unary", "unary-res", "unary-norelu", "unary-norelu-res", "simple", "simple2", "resnetb-projected", "resnetb-identity-shortcut",
           "resnetb-identity-unary1", "resnetb-strided-projected", "resnetb-strided-identity-shortcut", "decoder-step"]


@functools.lru_cache(maxsize=None)
def _batches(gpu):
    b = T._golden_batch()
    return b.to(gpu), _batch64(b)


@pytest.mark.parametrize("name", _BLOCKS)
def test_block_folded_vs_cpu_float64(gpu, name):
    from oracle import kpconv_ref
    from weasal_amd import fused
    cases = _block_cases(gpu)
    assert sorted(cases) == sorted(_BLOCKS)
    make, call, shapes, nsites = cases[name]
    batch_g, batch_c = _batches(gpu)
    batch_g.activate()
    g = torch.Generator().manual_seed(41)
    xs = [torch.randn(s, generator=g) for s in shapes]
    np.random.seed(0), torch.manual_seed(0)
    block = _move_bn(make('points')).eval()
    np.random.seed(0), torch.manual_seed(0)
    refmode = _move_bn(make('reference')).eval().to(gpu)
    block64 = copy.deepcopy(block).double()
    block = block.to(gpu)
    xg = [x.to(gpu) for x in xs]
    assert fused.bn_live(block) and not fused.bn_declines(block)
    with torch.no_grad():
        with kpconv_ref.cpu_reference_mode():
            ref = call(block64, batch_c, [x.double() for x in xs])
        folded, launches, folds = _counted(lambda: call(block, batch_g, xg))
        with _fold_switch(False):
            assert fused.bn_declines(block)
            off, launches_off, folds_off = _counted(lambda: call(block, batch_g, xg))
        _, launches_ref, folds_ref = _counted(lambda: call(refmode, batch_g, xg))
        # inside a network's forward the block looks its operands up: nothing is folded on the spot
        batch_g.bn_folds = fused.fold_network(block, xg[0])
        try:
            looked_up, launches_in, folds_in = _counted(lambda: call(block, batch_g, xg))
        finally:
            batch_g.bn_folds = None
    print("%s: launches folded %d (+ %d fold), fold-off %d, reference mode %d" % (name, launches, folds, launches_off, launches_ref))
    _held("block/" + name, folded, off, ref)
    assert folds == nsites and folds_off == 0 and folds_ref == 0 and folds_in == 0
    assert launches == launches_ref == launches_in and launches_off > launches        # the fused route was taken
    assert torch.equal(looked_up, folded)


# ------------------------------------------------------------------------------------------------------------------
# 5. - 8. networks
# ------------------------------------------------------------------------------------------------------------------
def _points_net_after_two_steps(gpu):
    """the 'points' KPFCNN of the existing test after two training steps on the golden batch (statistics and gamma have moved)
    -> (net in train(), cfg, batch, [the two steps' logits])"""
    from weasal_amd.trainer import make_optimizer, train_step
    cfg = T._net_config('points')
    net = T._make_net('points').to(gpu).train()
    batch = T._golden_batch().to(gpu)
    opt = make_optimizer(net, cfg)
    outs = [train_step(net, opt, batch, cfg)[1].detach().clone() for _ in range(2)]
    return net, cfg, batch, outs, opt


def _eval_logits(net, batch, cfg):
    net.eval()
    with torch.no_grad():
        return net(batch, cfg)


def _reference_mode_bits(gpu):
    cfg = T._net_config('reference')
    net = T._make_net('reference').to(gpu).train()
    batch = T._golden_batch().to(gpu)
    out, launches, folds = _counted(lambda: net(batch, cfg))
    out.square().mean().backward()
    grads = torch.cat([p.grad.reshape(-1) for p in net.parameters() if p.grad is not None])
    ev, _, folds_ev = _counted(lambda: _eval_logits(net, batch, cfg))
    return {"reference_out": out.detach().cpu(), "reference_grads": grads.cpu(), "reference_eval": ev.cpu(), "reference_folds": folds + folds_ev}


def _child_bits(gpu):
    net, cfg, batch, outs, _ = _points_net_after_two_steps(gpu)
    res = {"points_train_%d" % i: o.cpu() for i, o in enumerate(outs)}
    res["points_eval"] = _eval_logits(net, batch, cfg).cpu()
    res.update(_reference_mode_bits(gpu))
    return res


@functools.lru_cache(maxsize=None)
def _child(switch):
    """_child_bits in a fresh process with WEASAL_BN_FOLD = switch"""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bits.pt")
        env = {k: v for k, v in os.environ.items() if k != "WEASAL_BN_FOLD"}
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(env, WEASAL_BN_FOLD=switch), capture_output=True,
                              text=True, timeout=600)
        assert proc.returncode == 0, proc.stdout + proc.stderr
        return torch.load(path)


def test_network_folded_vs_cpu_float64_and_the_switch(gpu):
    from oracle import kpconv_ref
    from weasal_amd import fused, ops
    assert ops.BN_FOLD and "WEASAL_BN_FOLD" not in os.environ
    net, cfg, batch, outs, _ = _points_net_after_two_steps(gpu)
    with kpconv_ref.cpu_reference_mode():
        ref = _eval_logits(_copy64(T._make_net('points'), net), _batch64(batch), cfg)
    folded, launches, folds = _counted(lambda: _eval_logits(net, batch, cfg))
    with _fold_switch(False):
        off, launches_off, folds_off = _counted(lambda: _eval_logits(net, batch, cfg))
    refnet = T._make_net('reference').to(gpu)
    _, launches_ref, folds_ref = _counted(lambda: _eval_logits(refnet, batch, T._net_config('reference')))
    nsites = sum(bn.foldable() for _, _, bn in fused.network_sites(net))
    print("KPFCNN: %d sites; launches per forward folded %d + %d fold, fold-off %d, reference mode %d" % (nsites, launches, folds, launches_off, launches_ref))
    _held("network/KPFCNN", folded, off, ref)
    assert nsites == 21 and folds == -(-nsites // R.WS_BN_FOLD_MAX) and folds_off == 0 and folds_ref == 0
    assert launches == launches_ref and launches_off > launches
    assert getattr(batch, "bn_folds", None) is None                        # nothing is kept beyond the forward
    # WEASAL_BN_FOLD=0 in a fresh process: the parent commit's evaluation route, bit for bit
    child = _child("0")
    assert torch.equal(child["points_eval"], off.cpu())
    assert not torch.equal(folded.cpu(), off.cpu())
    # 'points' in training mode does not see the switch
    for i, o in enumerate(outs):
        assert torch.equal(child["points_train_%d" % i], o.cpu()), i


def test_reference_mode_is_untouched(gpu):
    """reference mode: zero fold launches, and the same bits with WEASAL_BN_FOLD unset (this process) and 0 (a fresh one)"""
    here, child = _reference_mode_bits(gpu), _child("0")
    assert here["reference_folds"] == 0 and child["reference_folds"] == 0
    for k in ("reference_out", "reference_grads", "reference_eval"):
        assert torch.equal(here[k], child[k]), k


def _small_mprm(gpu):
    import test_mprm_head_gpu as M
    from weasal_amd import pyramid, synthetic
    from weasal_amd.architectures import KPFCNN_mprm
    nets = {}
    for mode in ("points", "reference"):
        cfg = M._small_config()
        if mode == "points":
            cfg.batch_norm_mode = "points"
        np.random.seed(5), torch.manual_seed(5)
        nets[mode] = (_move_bn(KPFCNN_mprm(cfg, np.arange(cfg.num_classes), [])), cfg)
        with torch.no_grad():
            for name, p in nets[mode][0].named_parameters():
                if name.endswith("gamma"):
                    p.fill_(0.37)
    cfg = nets["points"][1]
    wl = synthetic.WORKLOADS["vaihingen_wl"]
    pts, feats, labels, lens = synthetic.make_inputs(4242, 2, 1500, 3.2, cfg.in_features_dim)
    region, region_lb, cloud_lb, centers = synthetic.make_weak_labels(9, pts, labels, lens, num_classes=cfg.num_classes)
    centers[:, 2] = (0.8, -1.1)
    np.random.seed(31)
    batch = pyramid.build_batch(cfg, torch.from_numpy(pts).to(gpu), torch.from_numpy(feats).to(gpu), torch.from_numpy(labels).to(gpu), lens,
                                wl["limits"])
    batch.center_pts = torch.from_numpy(centers).to(gpu)
    batch.cloud_lb = torch.from_numpy(cloud_lb).to(gpu)
    batch.region, batch.region_lb = M._regions_csr(region, region_lb, lens, gpu), None
    return nets, batch


def test_mprm_network_folded_vs_cpu_float64(gpu):
    from oracle import kpconv_ref
    from weasal_amd import fused
    from weasal_amd.trainer import make_optimizer, train_step_weak
    nets, batch = _small_mprm(gpu)
    net, cfg = nets["points"]
    net = net.to(gpu).train()
    opt = make_optimizer(net, cfg)
    for _ in range(2):
        loss, _ = train_step_weak(net, opt, batch, cfg)
        assert loss is not None and bool(torch.isfinite(loss))
    from weasal_amd.architectures import KPFCNN_mprm
    with kpconv_ref.cpu_reference_mode():
        ref = _eval_logits(_copy64(KPFCNN_mprm(cfg, np.arange(cfg.num_classes), []), net), _batch64(batch, ("center_pts",)), cfg)
    folded, launches, folds = _counted(lambda: _eval_logits(net, batch, cfg))
    with _fold_switch(False):
        off, launches_off, folds_off = _counted(lambda: _eval_logits(net, batch, cfg))
    refnet, refcfg = nets["reference"]
    _, launches_ref, folds_ref = _counted(lambda: _eval_logits(refnet.to(gpu), batch, refcfg))
    nsites = sum(bn.foldable() for _, _, bn in fused.network_sites(net))
    print("KPFCNN_mprm: %d sites; launches per forward folded %d + %d fold, fold-off %d, reference mode %d" % (nsites, launches, folds, launches_off, launches_ref))
    _held("network/KPFCNN_mprm", folded, off, ref)
    assert folds == -(-nsites // R.WS_BN_FOLD_MAX) and folds_off == 0 and folds_ref == 0
    assert launches == launches_ref and launches_off > launches


def test_frozen_statistics_with_gradients(gpu):
    """net.train() with every nn.BatchNorm1d in eval(): one train_step against the CPU reference; the fused training routes run"""
    from oracle import kpconv_ref
    from weasal_amd import fused
    from weasal_amd.trainer import make_optimizer, train_step
    cfg = T._net_config('points')
    cfg.grad_clip_norm = 100.0              # (far above every gradient: the clamp inside the update changes nothing)
    net_g, net_c = T._make_net('points'), T._make_net('points')
    net_c.load_state_dict(net_g.state_dict())
    net_g.to(gpu).train(), net_c.train()
    for net in (net_g, net_c):
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.eval()
    buffers = {k: v.clone() for k, v in net_g.state_dict().items() if "running_" in k or k.endswith("num_batches_tracked")}
    batch_g, batch_c = T._golden_batch().to(gpu), T._golden_batch()
    opt_g, opt_c = make_optimizer(net_g, cfg), make_optimizer(net_c, cfg)
    hits = fused.gate_link_hits
    (loss_g, out_g), launches, folds = _counted(lambda: train_step(net_g, opt_g, batch_g, cfg))
    with kpconv_ref.cpu_reference_mode():
        loss_c, out_c = train_step(net_c, opt_c, batch_c, cfg)
    dl = abs(float(loss_g.detach()) - float(loss_c.detach()))
    print("frozen statistics: logits %.3e  loss %.3e  fold launches %d  gate link hits %d" % (T._rel(out_g, out_c), dl, folds, fused.gate_link_hits - hits))
    assert T._rel(out_g, out_c) < 1e-4 and dl < 1e-4 * max(abs(float(loss_c.detach())), 1.0)
    assert folds == 2 and fused.gate_link_hits > hits                      # one fold launch each way; the fused routes ran
    grads_c = {k: p.grad for k, p in net_c.named_parameters()}
    worst = ("", 0.0)
    for k, p in net_g.named_parameters():
        assert (p.grad is None) == (grads_c[k] is None), k
        if p.grad is None:
            continue
        e = T._rel(p.grad, grads_c[k])
        worst = max(worst, (k, e), key=lambda kv: kv[1])
        assert e < 1e-4, (k, e)
    print("worst gradient: %s %.3e" % worst)
    assert any(k.endswith("batch_norm.weight") and p.grad is not None and bool(p.grad.any()) for k, p in net_g.named_parameters())
    sd_c = net_c.state_dict()
    for k, v in net_g.state_dict().items():
        if k in buffers:
            assert torch.equal(v, buffers[k]), k                           # statistics frozen: buffers and counters untouched
        else:
            assert T._rel(v, sd_c[k]) < 1e-4, k


def test_no_stale_weights_after_a_training_step(gpu):
    """evaluation, one ordinary training step (FusedSGD and ws_bn_fwd write through raw pointers: no version counter moves),
    evaluation again: the second forward sees the new parameters and statistics"""
    from oracle import kpconv_ref
    from weasal_amd.trainer import FusedSGD, train_step
    net, cfg, batch, _, opt = _points_net_after_two_steps(gpu)
    assert isinstance(opt, FusedSGD)
    first = _eval_logits(net, batch, cfg).clone()
    net.train()
    train_step(net, opt, batch, cfg)
    second = _eval_logits(net, batch, cfg)
    with _fold_switch(False):
        off = _eval_logits(net, batch, cfg)
    with kpconv_ref.cpu_reference_mode():
        ref = _eval_logits(_copy64(T._make_net('points'), net), _batch64(batch), cfg)
    _held("stale/second forward", second, off, ref)
    assert not torch.equal(first, second)
    stale = float((first.double().cpu() - ref).abs().max())
    print("first forward against the new state: %.3e" % stale)
    assert stale > 10 * float((second.double().cpu() - ref).abs().max())


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from weasal_amd import ops as _ops
    assert _ops.BN_FOLD == (os.environ.get("WEASAL_BN_FOLD", "1") != "0")
    torch.save(_child_bits(torch.device("cuda:0")), sys.argv[1])
