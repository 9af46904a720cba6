"""CPU: the float64 reference of the block and decoder-step calls (oracle/block_ref.py) before it judges a kernel --
every case of the table finds a decided seed (no LeakyReLU pre-activation within four comparison bounds of zero), the
branch ledger takes every value of every predicate of weasal_amd/csrc/blocks.hip, every flag a case turns on moves its
tensor by more than 100 bounds, and the restatement agrees with the project's own module classes under
oracle.kpconv_ref.cpu_reference_mode (the oracle the goldens pin)."""
import types

import numpy as np
import pytest
import torch

from oracle import block_ref as B
from oracle import kpconv_ref

CPU_BUILT = [c.name for c in B.KP_CASES + B.UP_CASES if getattr(c, "geometry", "cpu") == "cpu"]


@pytest.mark.parametrize("name", CPU_BUILT)
def test_builder_finds_a_decided_seed_and_the_flags_leave_a_trace(name):
    b = B.build(name)                     # (raises when 64 seeds are not enough, or a pooled maximum ties between real rows)
    c = b.case
    assert c.base_seed <= b.seed < c.base_seed + B.TRIES
    assert not B.undecided(b.ref64["pre"], b.ref32["pre"])
    assert B.build(name) is b             # one build per case: both test files see the same inputs
    for k in b.names:
        assert b.ref64[k] is not None and bool(torch.isfinite(b.ref64[k]).all()), k
        assert float(b.ref64[k].abs().max()) > 0, k
        assert b.err32[k] <= 1e-4 * float(b.ref64[k].abs().max()), (k, b.err32[k])      # float32 is a sane yardstick here
    sens = B.sensitivity(b)
    assert set(sens) == {e for e, _ in B.effects(c)}
    for effect, (moved, need) in sens.items():
        print("%s seed %d: without %-12s its tensor moves by %.3e (100 bounds = %.3e)" % (name, b.seed, effect, moved, need))
        assert moved > need, (name, effect, moved, need)


def test_the_seed_is_a_function_of_the_case_alone():
    name = "resnet_64_128"
    b = B.build(name)
    again = B.kp_inputs(b.case, b.seed, B.kp_geometry(b.case))
    for k, v in b.inputs.items():
        assert (v is None and again[k] is None) or torch.equal(v, again[k]), k
    g = B.kp_geometry(b.case)
    assert torch.equal(g.inds, b.geo.inds) and torch.equal(g.s_pts, b.geo.s_pts)


def test_geometry_has_the_edges_the_cases_name():
    for c in B.KP_CASES:
        if c.geometry != "cpu":
            continue
        g = B.kp_geometry(c)
        ns = g.s_pts.shape[0]
        assert g.inds.shape[0] == c.nq and int(g.inds.max()) == ns and int(g.inds.min()) >= 0
        assert bool((g.inds == ns).any(1).sum() >= c.nq // 4)                  # rows padded with the shadow index
        assert (g.inds.shape[1] == 256) == c.wide_inds and (c.wide_inds or 8 <= g.inds.shape[1] <= 128)
        assert bool((g.inds == ns).all(1).any()) == c.shadow_row
        assert float(g.kp.norm(dim=1).max()) < 0.7 * g.radius
        if c.rows_sorted:
            assert g.search_radius > 1.2 * g.radius
            sp = torch.cat([g.s_pts, torch.full((1, 3), 1e6)])
            d = (sp[g.inds] - g.q_pts[:, None, :]).double().norm(dim=2)
            assert bool((d[:, 1:] >= d[:, :-1]).all())                         # sorted by distance, as the hint vouches
    # a pooled maximum taken by the shadow row's zero, and an exact tie of a real 0.0 with it, both occur in the table
    wins = ties = 0
    for c in B.KP_CASES:
        if c.geometry == "cpu" and c.strided:
            b = B.build(c.name)
            w, t = B.shadow_pool_wins(c, b.geo, b.inputs)
            wins, ties = wins + w, ties + t
    assert wins > 0 and ties > 0, (wins, ties)


def test_ledger_takes_every_value_of_every_predicate():
    assert B.coverage(B.KP_CASES, B.KP_REQUIRED) == {}
    assert B.coverage(B.UP_CASES, B.UP_REQUIRED) == {}
    # the ledger's own rules at the values the issue names
    led = {c.name: B.ledger(c) for c in B.KP_CASES + B.UP_CASES}
    assert led["resnet_64_128"]["pair_in"] and led["resnet_64_128"]["pair_dz"] and led["resnet_64_128"]["gated2"]
    assert led["resnet_64_128"]["gate1"] == "x1" and led["resnet_64_128_bias"]["gate1"] == "none"
    assert not led["resnet_w1_offset"]["pair_in"] and not led["switch_group_rows_0"]["pair_in"]
    assert all(led["resnet_16_64_bias"]["in_place " + k] == "no: shape" for k in ("unary1", "unary2", "shortcut", "wk^T"))
    assert all(led["resnet_64_128"]["in_place " + k] == "yes" for k in ("unary1", "unary2", "shortcut", "wk^T"))
    assert led["strided_projection"]["arg_bytes"] and not led["strided_wide_inds"]["arg_bytes"] and not led["strided_feat_offset_add"]["arg_bytes"]
    assert led["infer_one_launch"]["forward"] == "one launch"
    assert {led[n]["forward"] for n in ("infer_two_launches", "infer_k9", "infer_k13")} == {"forward only: gather + product"}
    assert not led["simple_first_block_bias"]["need_dx1"] and led["resnet_first_block"]["need_dx1"]
    assert not led["resnet_no_unary1_first_block"]["need_dx1"]
    assert B.kp_ledger(B.CASES["strided_projection"], h=255)["arg_bytes"] and not B.kp_ledger(B.CASES["strided_projection"], h=256)["arg_bytes"]


def test_every_library_switch_is_held_at_zero_by_a_case():
    seen = {k for c in B.KP_CASES + B.UP_CASES for k, v in c.switches.items() if v == 0}
    assert seen == set(B.SWITCHES)


def _cfg():
    from weasal_amd import config as wcfg
    cfg = wcfg.DALESPLConfig()
    cfg.use_batch_norm = False             # BatchNormBlock is a learned bias: b1 / bk / b2 / bs are live
    return cfg


def _agree(tag, got, want):
    for k, w in want.items():
        err = float((got[k] - w).abs().max())
        print("%s %-6s |module - restatement| %.3e  max %.3e" % (tag, k, err, float(w.abs().max())))
        assert err <= 1e-5 * float(w.abs().max()), (tag, k, err)


@pytest.mark.parametrize("name", ["simple_first_block_bias", "resnet_64_128_bias", "strided_projection_bias"])
def test_restatement_agrees_with_the_module_classes(name):
    """SimpleBlock / ResnetBottleneckBlock of weasal_amd.blocks, evaluated by the CPU oracle, on the case's inputs (the
    module's own kernel points and extent go into the restatement)"""
    from weasal_amd import blocks
    b = B.build(name)
    c, t = b.case, b.inputs
    np.random.seed(3)
    torch.manual_seed(3)
    if c.kind == "simple":
        blk = blocks.SimpleBlock("simple", c.in_dim, 2 * c.out_dim, b.geo.radius, 0, _cfg())
        params = {"KPConv.weights": "wk", "batch_norm.bias": "bk"}
    else:
        blk = blocks.ResnetBottleneckBlock("resnetb_strided" if c.strided else "resnetb", c.in_dim, c.out_dim, b.geo.radius, 0, _cfg())
        params = {"unary1.mlp.weight": "w1", "unary1.batch_norm.bias": "b1", "KPConv.weights": "wk", "batch_norm_conv.bias": "bk",
                  "unary2.mlp.weight": "w2", "unary2.batch_norm.bias": "b2", "unary_shortcut.mlp.weight": "ws",
                  "unary_shortcut.batch_norm.bias": "bs"}
    named = dict(blk.named_parameters())
    assert set(params) == {k for k in named if k != "KPConv.kernel_points"}
    with torch.no_grad():
        for k, src in params.items():
            named[k].copy_(t[src])
    geo = types.SimpleNamespace(**vars(b.geo))
    geo.kp, geo.extent = blk.KPConv.kernel_points.detach().clone(), blk.KPConv.KP_extent
    batch = types.SimpleNamespace(points=[geo.s_pts, geo.q_pts], neighbors=[geo.inds], pools=[geo.inds])
    x = t["feat"].clone().requires_grad_(True)
    with kpconv_ref.cpu_reference_mode():
        out = blk(x, batch)
        out.backward(t["g"])
    got = {"out": out.detach(), "dfeat": x.grad}
    for k, src in params.items():
        got["d" + src] = named[k].grad
    plain = types.SimpleNamespace(**vars(c))
    plain.want_dfeat = True
    want = B.kpblock_ref(plain, geo, t, torch.float32)
    _agree(name, got, {k: want[k] for k in got})


def test_restatement_agrees_with_upsample_and_unary_block():
    from weasal_amd import blocks
    b = B.build("up_relu_bias")
    c, t = b.case, b.inputs
    torch.manual_seed(3)
    unary = blocks.UnaryBlock(c.c_up + c.c_skip, c.out_dim, False, 0)
    up = blocks.NearestUpsampleBlock(1)
    with torch.no_grad():
        unary.mlp.weight.copy_(t["w"])
        unary.batch_norm.bias.copy_(t["b"])
    batch = types.SimpleNamespace(upsamples=[b.geo.ups])
    xc, skip = t["xc"].clone().requires_grad_(True), t["skip"].clone().requires_grad_(True)
    with kpconv_ref.cpu_reference_mode():
        out = unary(torch.cat([up(xc, batch), skip], 1))
        out.backward(t["g"])
    got = {"out": out.detach(), "dxc": xc.grad, "dskip": skip.grad, "dw": unary.mlp.weight.grad, "db": unary.batch_norm.bias.grad}
    want = B.upunary_ref(c, b.geo, t, torch.float32)
    _agree("up_relu_bias", got, {k: want[k] for k in got})
