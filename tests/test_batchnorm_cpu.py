"""CPU: batch normalisation over the points (include/weasal_hip.h: ws_bn_*; weasal_amd/csrc/batchnorm.hip) without a device.

1. tests/bn_ref.py in float64 against torch autograd of F.batch_norm + add + F.leaky_relu in float64 (1e-12 relative):
   training and evaluation, with and without residual and activation, running statistics and num_batches_tracked after two
   calls.
2. The row table of bn_ref through the reporter ws_bn_variant: the shape rows each name a branch of their own, and every
   branch class the plan function produces over a sweep of shapes is named by some row.
3. A negative control: seven wrong restatements (bn_ref.MUTATIONS) are each rejected by the bound on at least one row.
4. Argument checks of the entries (they need no device), the ops wrapper's refusals, parameters.txt, and the modules: a small
   KPFCNN in 'points' mode on CPU tensors (the framework route) differs from reference mode and trains its gamma.
"""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_ref as R
from conftest import golden


def _L():
    from weasal_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------------------------
# 1. the restatement against autograd
# ------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("training", (True, False))
@pytest.mark.parametrize("residual", (False, True))
@pytest.mark.parametrize("act", (0, 1))
def test_restatement_is_torch_batch_norm_in_float64(training, residual, act):
    g = torch.Generator().manual_seed(5)
    n, c, m = 203, 7, 0.02
    gamma, beta = (torch.rand(c, generator=g) + 0.5).double(), torch.randn(c, generator=g).double()
    gamma[0], gamma[1] = 0.0, -1.3
    rm, rv, nbt = torch.randn(c, generator=g).double(), (torch.rand(c, generator=g) + 0.5).double(), 0
    t_rm, t_rv = rm.clone(), rv.clone()
    for call in range(2):
        y = (torch.randn(n, c, generator=g) * 3 + 1).double().requires_grad_(True)
        res = torch.randn(n, c, generator=g).double().requires_grad_(True) if residual else None
        dout = torch.randn(n, c, generator=g).double()
        tg, tb = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        z = F.batch_norm(y, t_rm, t_rv, tg, tb, training, m, R.EPS)
        if residual:
            z = z + res
        want = F.leaky_relu(z, R.SLOPE) if act else z
        want.backward(dout)
        f = R.forward(y.detach(), gamma, beta, rm, rv, nbt, R.EPS, training, m, res.detach() if residual else None, act, R.SLOPE)
        b = R.backward(dout, f["out"], y.detach(), gamma, f["save_mean"], f["save_rstd"], training, act, R.SLOPE)
        rm, rv, nbt = f["running_mean"], f["running_var"], f["num_batches_tracked"]
        assert _rel(f["out"], want.detach()) < 1e-12
        assert _rel(b["dy"], y.grad) < 1e-12 and _rel(b["dgamma"], tg.grad) < 1e-12 and _rel(b["dbeta"], tb.grad) < 1e-12
        if residual:
            assert _rel(b["dresidual"], res.grad) < 1e-12
        assert _rel(rm, t_rm) < 1e-12 and _rel(rv, t_rv) < 1e-12
    assert nbt == (2 if training else 0)
    # the module does the same bookkeeping (num_batches_tracked is the module's, not F.batch_norm's)
    bn = torch.nn.BatchNorm1d(c, momentum=m).double().train(training)
    bn(torch.randn(n, c, generator=g).double()), bn(torch.randn(n, c, generator=g).double())
    assert int(bn.num_batches_tracked) == nbt


# ------------------------------------------------------------------------------------------------------------------
# 2. the branch table
# ------------------------------------------------------------------------------------------------------------------
_BASE = 0x7f0000001000          # never read: the reporter looks at NULL-ness and alignment only


def _variant(n, c, training=1, act=1, residual=True, pad=0, off=None, dres=True, backward=0, expect=0):
    lib = _L().lib()
    buf = C.create_string_buffer(512)
    ld = c + pad

    def p(name, present=True):
        return C.c_void_p(_BASE + (4 if off == name else 0)) if present else None
    if backward:
        rc = lib.ws_bn_variant(1, n, c, p("y"), ld, p("out", bool(act)), ld, p("dresidual", dres), ld, p("dout"), ld, p("dy"), ld,
                               int(training), int(act), buf, 512)
    else:
        rc = lib.ws_bn_variant(0, n, c, p("y"), ld, p("out"), ld, p("residual", residual), ld, None, 0, None, 0, int(training),
                               int(act), buf, 512)
    assert rc == expect, (rc, lib.ws_last_error())
    return buf.value.decode()


def _row_variant(row, backward):
    return _variant(row["n"], row["c"], row["training"], row["act"], row["residual"], row["pad"], row["off"], row["dres"], backward)


_TEXT = re.compile(r"(\S+)<V=(\d)> (vector|scalar) rows=(\d+) chunks=(\d+) depth=(\d) tile=(\d+) lanes=(\d+) ctiles=(\d+) "
                   r"mode=(training|evaluation) residual=([01]) act=([01])$")


def _klass(text):
    """the branch classes of a reporter text.  The factors that decide which code runs are independent of one another in
    the kernels -- the column path V is a template argument; the merge depth concerns the finish kernel alone; column
    tiles are grid.y; a narrow tile idles threads; the rows per thread are trips of one loop -- so a class is one
    (kernel family, V, factor, value), not the product of all factors."""
    m = _TEXT.match(text)
    assert m, text
    kernels, v, path, rows, chunks, depth, tile, lanes, ctiles = m.group(1), int(m.group(2)), m.group(3), *map(int, m.groups()[3:9])
    assert (v == 4) == (path == "vector") and rows % lanes == 0
    per_thread = rows // lanes
    factors = {"depth": depth, "tiles": "several" if ctiles > 1 else "one", "tile": "full" if tile == 64 * v else "narrow",
               "rows": "1" if per_thread == 1 else ("<=8" if per_thread <= 8 else ">8")}
    return {(kernels, v, name, value) for name, value in factors.items()}


def test_every_shape_row_names_a_branch_of_its_own():
    seen = {}
    for row in R.SHAPE_ROWS + R.MODE_ROWS + R.PITCH_ROWS:
        m = _TEXT.match(_row_variant(row, 0))
        last = row["n"] - (int(m.group(5)) - 1) * int(m.group(4))        # rows of the last chunk: which lanes idle, which run short
        key = (_row_variant(row, 0), _row_variant(row, 1), last, row["dres"], row["momentum"], row["pad"])
        assert key not in seen, (row["id"], seen[key])
        seen[key] = row["id"]
        assert _TEXT.match(key[0]) and _TEXT.match(key[1]), key
    # what the ids claim
    assert "rows=32 chunks=1 depth=0" in _row_variant(R.BY_ID["n32-c32"], 0) and "chunks=2 depth=1" in _row_variant(R.BY_ID["n33-c32"], 0)
    assert "chunks=64 depth=1" in _row_variant(R.BY_ID["n2048-c32"], 0) and "chunks=65 depth=2" in _row_variant(R.BY_ID["n2049-c32"], 0)
    assert "rows=64 " in _row_variant(R.BY_ID["n16385-c32-two-rows-per-thread"], 1)
    assert "rows=256 " in _row_variant(R.BY_ID["n65539-c32-eight-rows-per-thread"], 0)
    cap = _TEXT.match(_row_variant(R.BY_ID["n700003-c3-chunk-cap"], 0))
    assert int(cap.group(4)) > 8 * int(cap.group(8)) and int(cap.group(5)) <= 1024          # rows raised by the cap
    assert "ctiles=4" in _row_variant(R.BY_ID["n284-c1024"], 0) and "vector" in _row_variant(R.BY_ID["n284-c1024"], 0)
    assert "scalar" in _row_variant(R.BY_ID["n65-c32-pitch-plus1-scalar"], 0) and "vector" in _row_variant(R.BY_ID["n65-c32-pitch-plus4"], 0)
    assert _row_variant(R.BY_ID["n257-c32-eval-res0-act0"], 0).startswith("bn_apply_fwd_kernel<")


def test_one_pointer_off_alignment_takes_the_scalar_path():
    for row in R.ALIGN_ROWS:
        forward = row["off"] in ("y", "out", "residual")
        assert ("scalar" in _row_variant(row, 0)) == forward, row["id"]
        assert ("scalar" in _row_variant(row, 1)) == (row["off"] != "residual"), row["id"]        # (out is read for the gate)
        assert "vector" in _row_variant(dict(row, off=None), 0) and "vector" in _row_variant(dict(row, off=None), 1)


def test_every_branch_class_of_the_plan_is_named_by_a_row():
    named = set()
    for row in R.ROWS:
        named |= _klass(_row_variant(row, 0)) | _klass(_row_variant(row, 1))
    reachable = {}
    ns = sorted(set(list(range(1, 70)) + [255, 256, 257, 1000, 2048, 2049, 4099, 8191, 16385, 33000, 65539, 90001, 300000, 700003]))
    for c in (1, 2, 3, 4, 8, 9, 16, 32, 45, 64, 128, 130, 255, 256, 257, 260, 261, 512, 1024):
        for n in ns:
            if n * c > 70000 * 32:        # the table's size limit
                continue
            for training in (1, 0):
                if training and n == 1:
                    continue
                for backward in (0, 1):
                    for k in _klass(_variant(n, c, training, backward=backward)):
                        reachable.setdefault(k, (n, c, training, backward))
    missing = {k: v for k, v in reachable.items() if k not in named}
    assert not missing, missing


# ------------------------------------------------------------------------------------------------------------------
# 3. the bound rejects wrong kernels
# ------------------------------------------------------------------------------------------------------------------
def test_float32_restatement_is_inside_its_own_bound():
    for row_id in R.CPU_ROWS:
        _, given, r64, err32 = R.case(row_id)
        got = R.evaluate(R.BY_ID[row_id], torch.float32, given_out=given)
        assert not R.violations(got, r64, err32), row_id


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_bound_rejects_a_wrong_restatement(mutation):
    rejected = []
    for row_id in R.CPU_ROWS:
        _, given, r64, err32 = R.case(row_id)
        got = R.evaluate(R.BY_ID[row_id], torch.float32, given_out=given, mutation=mutation)
        if R.violations(got, r64, err32):
            rejected.append(row_id)
    print("%s: rejected on %d of %d rows" % (mutation, len(rejected), len(R.CPU_ROWS)))
    assert rejected, mutation


# ------------------------------------------------------------------------------------------------------------------
# 4. argument checks, wrapper, configuration, modules
# ------------------------------------------------------------------------------------------------------------------
def _fwd(lib, n=8, c=4, ldy=4, ldo=4, ldr=4, training=1, act=1, eps=1e-5, y=_BASE, out=_BASE, gamma=_BASE, rm=_BASE, save=_BASE,
         scratch=_BASE, residual=None):
    v = C.c_void_p
    return lib.ws_bn_fwd(v(y) if y else None, n, c, ldy, v(gamma) if gamma else None, v(_BASE), eps, training, 0.02, v(rm) if rm else None,
                         v(_BASE), None, residual, ldr, act, 0.1, v(out) if out else None, ldo, v(save) if save else None,
                         v(save) if save else None, v(scratch) if scratch else None, None)


def _bwd(lib, n=8, c=4, ld=4, training=1, act=1, out=_BASE, dgamma=_BASE, save=_BASE, rm=None, scratch=_BASE, dy=_BASE):
    v = C.c_void_p
    return lib.ws_bn_bwd(v(_BASE), ld, v(out) if out else None, ld, v(_BASE), ld, n, c, v(_BASE), v(save) if save else None,
                         v(save) if save else None, v(rm) if rm else None, v(rm) if rm else None, 1e-5, training, act, 0.1,
                         v(dy) if dy else None, ld, None, ld, v(dgamma) if dgamma else None, v(_BASE), v(scratch) if scratch else None,
                         None)


def test_argument_checks_need_no_device():
    lib = _L().lib()
    INVALID, UNSUPPORTED = 1, 2
    assert {"ws_bn_scratch_bytes", "ws_bn_fwd", "ws_bn_bwd", "ws_bn_variant"} <= set(_L().SIGNATURES)
    # sizes
    assert lib.ws_bn_scratch_bytes(-1, 4) == -1 and lib.ws_bn_scratch_bytes(5, 0) == -1 and lib.ws_bn_scratch_bytes(0, 4) == 0
    assert lib.ws_bn_scratch_bytes(400000, 32) >= 4 * 4 * 32 * ((400000 + 415) // 416)
    for n, c in ((2, 1), (257, 9), (284, 1024), (16385, 32), (700003, 3)):      # covers both column paths' chunk counts
        for off in (None, "y"):
            chunks = int(_TEXT.match(_variant(n, c, off=off)).group(5))
            assert lib.ws_bn_scratch_bytes(n, c) >= 4 * 4 * c * chunks
    assert _fwd(lib, n=-1) == INVALID and _fwd(lib, c=0) == INVALID and _fwd(lib, c=(1 << 20) + 1, ldy=1 << 21, ldo=1 << 21) == UNSUPPORTED
    assert _fwd(lib, ldy=3) == INVALID and _fwd(lib, ldo=3) == INVALID and _fwd(lib, residual=C.c_void_p(_BASE), ldr=3) == INVALID
    assert _fwd(lib, act=2) == INVALID and _fwd(lib, eps=-1.0) == INVALID
    assert _fwd(lib, n=1) == INVALID and b"more than 1" in lib.ws_last_error()      # training with a single row, as torch refuses it
    for missing in ("y", "out", "gamma", "rm", "save", "scratch"):
        assert _fwd(lib, **{missing: 0}) == INVALID, missing
    assert _fwd(lib, n=0, y=0, out=0, save=0, scratch=0) == 0                     # nothing to do, nothing touched
    assert _bwd(lib, n=-1) == INVALID and _bwd(lib, c=0) == INVALID and _bwd(lib, ld=3) == INVALID and _bwd(lib, act=3) == INVALID
    assert _bwd(lib, n=1) == INVALID and _bwd(lib, dgamma=0) == INVALID and _bwd(lib, out=0) == INVALID and _bwd(lib, scratch=0) == INVALID
    assert _bwd(lib, dy=0) == INVALID and _bwd(lib, save=0) == INVALID and _bwd(lib, training=0, save=0, rm=0) == INVALID
    # the reporter
    assert _variant(0, 4) == "none (n == 0)" and _variant(0, 4, backward=1) == "memset (n == 0)"
    _variant(1, 4, training=1, expect=INVALID)
    assert "mode=evaluation" in _variant(1, 4, training=0)


def test_ops_wrapper_refuses_what_the_kernels_do_not_take():
    from weasal_amd import ops
    bn = torch.nn.BatchNorm1d(4)
    with pytest.raises(_L().WeasalHipError):
        ops.batch_norm_act(torch.zeros(5, 4), bn)                                  # CPU tensors, like every operator
    assert os.environ.get("WEASAL_BN_KERNELS", "1") == "0" or ops.BN_KERNELS


def test_block_modes_and_state_dict_keys():
    from weasal_amd.blocks import BatchNormBlock, UnaryBlock
    ref, pts = BatchNormBlock(6, True, 0.02), BatchNormBlock(6, True, 0.02, mode='points')
    assert ref.mode == 'reference' and not ref.live() and pts.live() and not BatchNormBlock(6, False, 0.02, mode='points').live()
    assert list(ref.state_dict()) == list(pts.state_dict())
    with pytest.raises(ValueError):
        BatchNormBlock(6, True, 0.02, mode='instance')
    x = torch.randn(9, 6)
    assert ref(x) is x                                                             # the reference's identity, untouched
    pts.train()
    want = F.batch_norm(x, None, None, pts.batch_norm.weight, pts.batch_norm.bias, True, 0.02, 1e-5)
    assert torch.allclose(pts(x), want, atol=1e-6) and int(pts.batch_norm.num_batches_tracked) == 1
    with pytest.raises(ValueError):
        pts(torch.randn(1, 6))                                                     # one row in training
    u = UnaryBlock(6, 5, True, 0.02, bn_mode='points')
    res = torch.randn(9, 5)
    y = F.linear(x, u.mlp.weight)
    want = F.leaky_relu(F.batch_norm(y, None, None, u.batch_norm.batch_norm.weight, u.batch_norm.batch_norm.bias, True) + res, 0.1)
    from oracle import kpconv_ref
    with kpconv_ref.cpu_reference_mode():
        got = u.forward_fused(x, residual=res, slope_override=0.1)
    assert torch.allclose(got, want, atol=1e-6)
    # the fused routes decline
    from weasal_amd import fused
    assert fused.bn_live(u) and not fused.bn_live(UnaryBlock(6, 5, True, 0.02)) and not fused.bn_live(UnaryBlock(6, 5, False, 0, bn_mode='points'))


def test_parameters_txt_defaults_unchanged_and_points_round_trips(tmp_path):
    from weasal_amd import config as wcfg
    for name, cls in (("dales", wcfg.DALESPLConfig), ("vaihingen", getattr(wcfg, "Vaihingen3DWLConfig", wcfg.DALESPLConfig))):
        cfg = cls()
        assert not hasattr(cfg, "batch_norm_mode")
        cfg.saving_path = str(tmp_path / name)
        os.makedirs(cfg.saving_path)
        cfg.save()
        text = open(os.path.join(cfg.saving_path, "parameters.txt")).read()
        assert "batch_norm_mode" not in text
        cfg.batch_norm_mode = 'points'
        cfg.saving_path = str(tmp_path / (name + "_points"))
        os.makedirs(cfg.saving_path)
        cfg.save()
        text_p = open(os.path.join(cfg.saving_path, "parameters.txt")).read()
        assert text_p == text + "batch_norm_mode = points\n"
        back = wcfg.Config().load(cfg.saving_path)
        assert back.batch_norm_mode == 'points'
        back.saving_path = str(tmp_path / (name + "_again"))
        os.makedirs(back.saving_path)
        back.save()
        assert open(os.path.join(back.saving_path, "parameters.txt")).read() == text_p
    # the golden files of the reference load without the key
    from conftest import GOLDEN
    assert not hasattr(wcfg.Config().load(os.path.join(GOLDEN, "params", "dales_pl")), "batch_norm_mode")


def _small_config(mode=None, **extra):
    from weasal_amd.config import Config

    class Cfg(Config):
        architecture = ['simple', 'resnetb', 'resnetb_strided', 'resnetb', 'resnetb_strided', 'resnetb',
                        'resnetb_strided', 'resnetb', 'resnetb_strided', 'resnetb',
                        'nearest_upsample', 'unary', 'nearest_upsample', 'unary',
                        'nearest_upsample', 'unary', 'nearest_upsample', 'unary']
        first_subsampling_dl = 0.24
        deform_radius = 6.0
        first_features_dim = 16
        in_features_dim = 4
        batch_norm_momentum = 0.02
        repulse_extent = 1.2
        dropout = 0
        saving = False
    cfg = Cfg()
    if mode is not None:
        cfg.batch_norm_mode = mode
    for k, v in extra.items():
        setattr(cfg, k, v)
    return cfg


def _golden_batch():
    g7 = golden("g7_pyramid.npz")
    t = lambda a: torch.from_numpy(np.asarray(a))
    b = types.SimpleNamespace()
    for name in ("points", "neighbors", "pools", "upsamples", "lengths"):
        setattr(b, name, [t(g7["%s_%d" % (name, l)]) for l in range(5)])
    b.features, b.labels = t(g7["features"]), t(g7["labels"])
    return b


def test_points_mode_network_normalises_and_trains_gamma():
    """the framework route on CPU tensors: 'points' changes the logits, gamma / beta get gradients, the running buffers
    move in train() and stand still in eval(); reference mode leaves all of that as it always was"""
    from oracle import kpconv_ref
    from weasal_amd.architectures import KPFCNN
    from weasal_amd.trainer import make_optimizer
    nets = {}
    for mode in ("reference", "points"):
        cfg = _small_config(mode if mode == "points" else None)
        np.random.seed(0)
        torch.manual_seed(0)
        nets[mode] = (KPFCNN(cfg, np.arange(9), []), cfg)
    nets["points"][0].load_state_dict(nets["reference"][0].state_dict())
    assert nets["points"][0].batch_norm_mode == 'points' and nets["reference"][0].batch_norm_mode == 'reference'
    outs = {}
    for mode, (net, cfg) in nets.items():
        net.train()
        b = _golden_batch()
        with kpconv_ref.cpu_reference_mode():
            out = net(b, cfg)
            net.loss(out, b.labels).backward()
        outs[mode] = out.detach()
    assert outs["points"].shape == outs["reference"].shape and not torch.allclose(outs["points"], outs["reference"], atol=1e-3)
    ref_named, pts_named = dict(nets["reference"][0].named_parameters()), dict(nets["points"][0].named_parameters())
    gammas = [k for k in pts_named if k.endswith("batch_norm.weight")]
    assert len(gammas) >= 20
    for k in gammas:
        assert ref_named[k].grad is None                                           # reference mode: dead, as always
        assert pts_named[k].grad is not None and pts_named[k.replace("weight", "bias")].grad is not None, k
    assert any(float(pts_named[k].grad.abs().max()) > 0 for k in gammas)
    bufs = dict(nets["points"][0].named_buffers())
    tracked = [k for k in bufs if k.endswith("num_batches_tracked")]
    assert all(int(bufs[k]) == 1 for k in tracked) and all(int(v) == 0 for k, v in nets["reference"][0].named_buffers()
                                                           if k.endswith("num_batches_tracked"))
    # the optimiser's two groups hold gamma and beta (neither is an 'offset' parameter)
    net, cfg = nets["points"]
    opt = make_optimizer(net, cfg)
    in_groups = {id(p) for g in opt.param_groups for p in g["params"]}
    assert all(id(pts_named[k]) in in_groups for k in gammas)
    # evaluation: running statistics, no side effects
    net.eval()
    before = {k: v.clone() for k, v in net.named_buffers()}
    with kpconv_ref.cpu_reference_mode(), torch.no_grad():
        ev = net(_golden_batch(), cfg)
    assert all(torch.equal(before[k], v) for k, v in net.named_buffers()) and not torch.allclose(ev, outs["points"], atol=1e-3)


def test_points_mode_refuses_bf16_rows():
    from weasal_amd.architectures import KPFCNN
    with pytest.raises(ValueError):
        KPFCNN(_small_config("points", feature_dtype='bf16'), np.arange(9), [])
    with pytest.raises(ValueError):
        KPFCNN(_small_config("instance"), np.arange(9), [])
    KPFCNN(_small_config("reference", feature_dtype='bf16'), np.arange(9), [])
