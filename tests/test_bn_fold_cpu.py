"""CPU: the restatement of the BN fold (tests/bn_fold_ref.py), the branch table of weasal_amd/csrc/bn_fold.hip through its
reporter, the argument checks of the three entries, the module predicates, and the negative control of the GPU bounds.

1. The restatement in float64 equals torch autograd through F.linear / the KPConv contraction composed with
   F.batch_norm(training=False), forward and backward, to 1e-12.
2. ws_bn_fold_variant: every row of bn_fold_ref.ROWS names a branch, and every branch of the plan (vector / scalar,
   row-sum / column-sum, wide / narrow column tile, one / several element chunks, one / several launches) is named by a row.
3. Argument checks need no device.
4. BatchNormBlock.foldable() for the four combinations of mode and training; fused.bn_live keeps its meaning, fused.bn_declines
   is the new predicate of the fused routes; CPU tensors never fold.
5. Four wrong restatements (var without eps, t without the mean term, dgamma without - mean * dt, the channel on the wrong
   axis) are each rejected by the bounds the GPU test applies, and the same arithmetic in float32 on the CPU is inside them.
"""
import ctypes as C
import re

import pytest
import torch
import torch.nn.functional as F

import bn_fold_ref as R


def _L():
    from weasal_amd import _lib
    return _lib


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


# ------------------------------------------------------------------------------------------------------------------
# 1. the restatement
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["linear", "kpconv"])
def test_restatement_is_torch_autograd_in_float64(kind):
    g = torch.Generator().manual_seed(5)
    n, c = 37, 6
    gamma = (torch.rand(c, generator=g) + 0.5).double().requires_grad_(True)
    beta = torch.randn(c, generator=g).double().requires_grad_(True)
    mean, var = torch.randn(c, generator=g).double(), (torch.rand(c, generator=g) + 0.3).double()
    gout = torch.randn(n, c, generator=g).double()
    if kind == "linear":
        w = torch.randn(c, 11, generator=g).double().requires_grad_(True)         # nn.Linear.weight [c, k]
        x = torch.randn(n, 11, generator=g).double()
        product = lambda weight: F.linear(x, weight)
        site = lambda t: t.reshape(1, c, 11)
    else:
        w = torch.randn(5, 4, c, generator=g).double().requires_grad_(True)       # KPConv weights [K, Ci, Co]
        wf = torch.randn(n, 5, 4, generator=g).double()
        product = lambda weight: wf.reshape(n, -1) @ weight.reshape(-1, c)
        site = lambda t: t.reshape(20, c, 1)
    want = F.batch_norm(product(w), mean, var, gamma, beta, False, 0.0, R.EPS)
    (want * gout).sum().backward()
    f = R.forward(site(w.detach()), gamma.detach(), beta.detach(), mean, var)
    wo = f["w_out"].reshape(w.shape).requires_grad_(True)
    to = f["t_out"].clone().requires_grad_(True)
    got = product(wo) + to
    (got * gout).sum().backward()
    b = R.backward(site(w.detach()), gamma.detach(), mean, var, site(wo.grad), to.grad)
    assert _rel(got.detach(), want.detach()) < 1e-12
    assert _rel(b["dw"].reshape(w.shape), w.grad) < 1e-12 and _rel(b["dgamma"], gamma.grad) < 1e-12 and _rel(b["dbeta"], beta.grad) < 1e-12
    # NULL gradients stand for zeros
    z = R.backward(site(w.detach()), gamma.detach(), mean, var, None, None)
    assert not z["dw"].any() and not z["dgamma"].any() and not z["dbeta"].any()


# ------------------------------------------------------------------------------------------------------------------
# 2. the branch table
# ------------------------------------------------------------------------------------------------------------------
_BASE = 0x7f0000001000          # never read: the reporter looks at NULL-ness and alignment only
_FWD = re.compile(r"bn_fold_fwd_kernel (vector|scalar) blocks=(\d+) launches=(\d+)$")
_BWD = re.compile(r"bn_fold_bwd_kernel (vector|scalar) (row-sum|column-sum) tile=(\d+) ew_blocks=(\d+) sum_blocks=(\d+) launches=(\d+)$")


def _variant(outer, c, inner, backward=0, off=None, count=1, expect=0):
    lib = _L().lib()
    buf = C.create_string_buffer(256)
    p = lambda name: C.c_void_p(_BASE + (4 if off == name else 0))
    rc = lib.ws_bn_fold_variant(backward, outer, c, inner, p("src"), p("dst"), count, buf, 256)
    assert rc == expect, (rc, lib.ws_last_error())
    return buf.value.decode()


def _classes(row):
    f = _FWD.match(_variant(row["outer"], row["c"], row["inner"], 0, row["off"]))
    b = _BWD.match(_variant(row["outer"], row["c"], row["inner"], 1, row["off"]))
    assert f and b, row["id"]
    n = row["outer"] * row["c"] * row["inner"]
    assert int(f.group(2)) == int(b.group(4)) == (n + 4095) // 4096 and f.group(1) == b.group(1)
    path, tile = b.group(2), int(b.group(3))
    assert (path == "column-sum") == (row["inner"] == 1) and int(b.group(5)) == (row["c"] + tile - 1) // tile
    return {("path", f.group(1)), ("sum", path), ("tile", tile), ("chunks", "one" if int(f.group(2)) == 1 else "several")}


def test_every_row_names_a_branch_and_every_branch_is_named_by_a_row():
    seen = set()
    for row in R.ROWS:
        seen |= _classes(row)
    want = {("path", "vector"), ("path", "scalar"), ("sum", "row-sum"), ("sum", "column-sum"), ("tile", 4), ("tile", 64), ("tile", 16),
            ("chunks", "one"), ("chunks", "several")}
    assert seen == want, seen ^ want
    # what decides the path: alignment of either pointer, and whether a quad of elements stays in known channels
    expect = {"linear-c32-k32": "vector", "linear-c32-k3": "scalar", "linear-c4-k1": "vector", "linear-c3-k1": "scalar",
              "kpconv-K9-ci4-co66": "scalar", "kpconv-K9-ci4-co32": "vector", "linear-c32-k32-src-off": "scalar",
              "linear-c32-k32-dst-off": "scalar", "kpconv-K15-ci4-co32-dst-off": "scalar", "mid-o3-c5-i7": "scalar"}
    for rid, path in expect.items():
        row = R.BY_ID[rid]
        assert _FWD.match(_variant(row["outer"], row["c"], row["inner"], 0, row["off"])).group(1) == path, rid
    assert _BWD.match(_variant(1023, 32, 1, 1)).group(3) == "64" and _BWD.match(_variant(1024, 32, 1, 1)).group(3) == "16"
    # the launches of a table
    cap = _L().ABI.constants["WS_BN_FOLD_MAX"]
    assert cap == R.WS_BN_FOLD_MAX
    for count, launches in ((1, 1), (cap, 1), (cap + 1, 2), (2 * cap + 1, 3)):
        assert int(_FWD.match(_variant(1, 32, 32, 0, count=count)).group(3)) == launches
        assert int(_BWD.match(_variant(1, 32, 32, 1, count=count)).group(6)) == launches
    assert _variant(1, 0, 32) == "none (c == 0) launches=0" and _variant(1, 32, 32, count=0) == "none (no sites) launches=0"


# ------------------------------------------------------------------------------------------------------------------
# 3. argument checks
# ------------------------------------------------------------------------------------------------------------------
def _table(count=1, outer=1, c=4, inner=4, eps=1e-5, null=(), backward=False):
    """the arguments of ws_bn_fold_fwd / _bwd for `count` equal sites whose pointers are never read"""
    arr = lambda name: None if name in null else (C.c_void_p * max(count, 1))(*[None if ("*" + name) in null else _BASE] * max(count, 1))
    sizes = [arr("w"), (C.c_int64 * max(count, 1))(*[outer] * max(count, 1)), (C.c_int32 * max(count, 1))(*[c] * max(count, 1)),
             (C.c_int64 * max(count, 1))(*[inner] * max(count, 1))]
    epsv = (C.c_float * max(count, 1))(*[eps] * max(count, 1))
    if backward:
        return sizes + [arr("gamma"), arr("mean"), arr("var"), epsv, arr("dw_out"), arr("dt_out"), arr("dw"), arr("dgamma"), arr("dbeta"),
                        count, None]
    return sizes + [arr("gamma"), arr("beta"), arr("mean"), arr("var"), epsv, arr("w_out"), arr("t_out"), count, None]


def test_argument_checks_need_no_device():
    L = _L()
    lib = L.lib()
    INVALID = 1
    assert {"ws_bn_fold_fwd", "ws_bn_fold_bwd", "ws_bn_fold_variant"} <= set(L.SIGNATURES)
    before = lib.ws_launch_count()
    for backward, entry in ((False, lib.ws_bn_fold_fwd), (True, lib.ws_bn_fold_bwd)):
        call = lambda **kw: entry(*_table(backward=backward, **kw))
        assert call(count=-1) == INVALID
        assert call(count=0) == 0 and call(count=0, null=("w", "gamma")) == 0            # nothing to do
        assert call(c=0) == 0 and call(c=0, count=R.WS_BN_FOLD_MAX + 3) == 0            # sites without channels: no launch
        assert call(c=-1) == INVALID and call(outer=0) == INVALID and call(inner=0) == INVALID and call(eps=-1.0) == INVALID
        assert call(outer=1 << 20, c=1 << 10, inner=2) == INVALID and b"too large" in lib.ws_last_error()
        for missing in ("w", "gamma", "mean", "var", "*w", "*gamma", "*mean", "*var"):
            assert call(null=(missing,)) == INVALID, missing
    for missing in ("beta", "w_out", "t_out", "*beta", "*w_out", "*t_out"):
        assert lib.ws_bn_fold_fwd(*_table(null=(missing,))) == INVALID, missing
    for missing in ("dw_out", "dt_out", "dw", "dgamma", "dbeta"):                    # the arrays; their entries may be NULL
        assert lib.ws_bn_fold_bwd(*_table(backward=True, null=(missing,))) == INVALID, missing
    assert lib.ws_bn_fold_bwd(*_table(backward=True, null=("*dw", "*dgamma", "*dbeta"))) == 0     # nothing asked for: passed over
    assert lib.ws_launch_count() == before
    # the reporter
    _variant(1, -1, 4, expect=INVALID), _variant(0, 4, 4, expect=INVALID), _variant(1, 4, 4, count=-1, expect=INVALID)
    assert lib.ws_bn_fold_variant(0, 1, 4, 4, None, None, 1, None, 0) == INVALID


def test_ops_wrapper_refuses_what_the_kernels_do_not_take():
    from weasal_amd import ops
    bn = torch.nn.BatchNorm1d(4).eval()
    assert ops.bn_fold([]) == []
    with pytest.raises(L_error()):
        ops.bn_fold([(torch.zeros(4, 3), 0, bn)])                                   # CPU tensors, like every operator
    with pytest.raises(ValueError):
        ops.bn_fold([(torch.zeros(4, 3), 0, torch.nn.BatchNorm1d(4, affine=False))])
    with pytest.raises(ValueError):
        ops.bn_fold([(torch.zeros(4, 3), 0, torch.nn.BatchNorm1d(4, track_running_stats=False))])


def L_error():
    return _L().WeasalHipError


# ------------------------------------------------------------------------------------------------------------------
# 4. the modules
# ------------------------------------------------------------------------------------------------------------------
def test_foldable_per_site_and_the_predicates_of_the_fused_routes():
    from weasal_amd import fused, ops
    from weasal_amd.blocks import BatchNormBlock, UnaryBlock
    assert ops.BN_FOLD and ops.BN_KERNELS
    for mode in ("reference", "points"):
        for training in (True, False):
            b = BatchNormBlock(6, True, 0.02, mode=mode).train(training)
            assert b.foldable() == (mode == "points" and not training), (mode, training)
    assert not BatchNormBlock(6, False, 0.02, mode="points").eval().foldable()        # a bias block
    # the flag is the BatchNorm1d's own: freezing that module alone folds it
    u, v = UnaryBlock(6, 5, True, 0.02, bn_mode="points"), UnaryBlock(6, 5, True, 0.02, bn_mode="points")
    u.train(), v.train()
    v.batch_norm.batch_norm.eval()
    assert not u.batch_norm.foldable() and v.batch_norm.foldable()
    # bn_live: "a BN of this block runs over the points", whatever its training flag; bn_declines: "... and does not fold"
    assert fused.bn_live(u) and fused.bn_live(v) and fused.bn_declines(u) and not fused.bn_declines(v)
    ref, bias = UnaryBlock(6, 5, True, 0.02), UnaryBlock(6, 5, False, 0, bn_mode="points")
    assert not fused.bn_live(ref) and not fused.bn_live(bias) and not fused.bn_declines(ref) and not fused.bn_declines(bias)
    # the switches
    for name in ("BN_FOLD", "BN_KERNELS"):
        setattr(ops, name, False)
        try:
            assert not v.batch_norm.foldable() and fused.bn_declines(v) and fused.bn_live(v)
        finally:
            setattr(ops, name, True)
    # CPU tensors never fold: the CPU network stays the reference
    x = torch.randn(9, 6)
    assert not fused.bn_folds(v.batch_norm, x)
    w, b = fused.folded_operands(v.mlp.weight, 0, v.batch_norm, None, x)
    assert w is v.mlp.weight and b is None
    w, b = fused.folded_operands(bias.mlp.weight, 0, bias.batch_norm, None, x)
    assert w is bias.mlp.weight and b is bias.batch_norm.bias
    from oracle import kpconv_ref
    v.eval()
    with kpconv_ref.cpu_reference_mode():
        got = v(x)
    bn = v.batch_norm.batch_norm
    want = F.leaky_relu(F.batch_norm(F.linear(x, v.mlp.weight), bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps), 0.1)
    assert torch.allclose(got, want, atol=1e-6)


def test_network_sites_and_no_fold_on_the_cpu():
    import numpy as np
    from weasal_amd import fused
    from weasal_amd.architectures import KPFCNN
    from weasal_amd.config import Config

    class Cfg(Config):
        architecture = ['simple', 'resnetb', 'resnetb_strided', 'resnetb', 'nearest_upsample', 'unary']
        first_features_dim = 16
        in_features_dim = 4
        batch_norm_mode = 'points'
    net = KPFCNN(Cfg(), np.arange(5), []).eval()
    sites = fused.network_sites(net)
    # simple: 1; resnetb 8 -> 32: unary1, conv, unary2, shortcut; strided 32 -> 64: 4; resnetb 64 -> 64: unary1, conv, unary2; the
    # decoder's unary; the two head blocks (bias blocks: listed, never foldable)
    assert len(sites) == 1 + 4 + 4 + 3 + 1 + 2
    assert sum(bn.foldable() for _, _, bn in sites) == len(sites) - 2
    for w, axis, bn in sites:
        assert w.shape[axis] == bn.in_dim
    assert fused.network_sites(net) is sites
    assert fused.fold_network(net, torch.zeros(3, 4)) is None                        # CPU rows: nothing folds, nothing is launched
    net.train()
    assert not any(bn.foldable() for _, _, bn in sites)


# ------------------------------------------------------------------------------------------------------------------
# 5. the bounds: inside for float32, outside for four wrong restatements
# ------------------------------------------------------------------------------------------------------------------
def test_float32_restatement_is_inside_the_bounds():
    worst = {}
    for row in R.ROWS:
        ins, ref = R.case(row["id"])
        got = R.reference(ins, torch.float32)
        assert not R.violations(got, ref, ins), (row["id"], R.violations(got, ref, ins))
        for key, unit in (("w_out", 4 * R.ULP * ref["w_out"].abs()), ("dw", 4 * R.ULP * ref["dw"].abs())):
            ratio = ((got[key].double() - ref[key]).abs() / unit.clamp(min=1e-300)).max()
            worst[key] = max(worst.get(key, 0.0), float(ratio))
    print("float32 on the CPU, worst fraction of the bound:", worst)
    assert all(v < 1.0 for v in worst.values())


_CATCHES = {"var_without_eps": ("w_out", "t_out", "dw", "dgamma"), "t_without_mean": ("t_out",), "dgamma_without_mean_dt": ("dgamma",),
            "wrong_axis": ("w_out",)}


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_bounds_reject_a_wrong_restatement(mutation):
    assert set(_CATCHES) == set(R.MUTATIONS)
    caught = 0
    for row in R.ROWS:
        ins, ref = R.case(row["id"])
        wrong = R.reference(ins, torch.float64, mutation)
        names = {name for name, _ in R.violations(wrong, ref, ins)}
        assert names <= set(_CATCHES[mutation]), (row["id"], names)
        caught += bool(names)
    print("%s: caught on %d of %d rows" % (mutation, caught, len(R.ROWS)))
    assert caught >= len(R.ROWS) // 2
