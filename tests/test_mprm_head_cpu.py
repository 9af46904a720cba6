"""CPU (no GPU needed): the float64 restatements of tests/mprm_head_ref.py against what the reference project itself calls
-- the split / mean / stack loop, the nested torch.max under autograd, BCEWithLogitsLoss(weight) under autograd,
clip_grad_norm_ + torch.optim.SGD -- in float64; the new header entries parse and bind; WEASAL_WL_ENDS = 0 selects the
framework paths; CPU tensors never reach the new operators."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mprm_head_ref as ref
from conftest import REPO

ENTRIES = ("ws_segment_mean_fwd", "ws_segment_mean_bwd", "ws_max_heads_fwd", "ws_max_heads_bwd", "ws_bce_heads_fwd",
           "ws_bce_heads_bwd", "ws_grad_norm_slots", "ws_grad_norm", "ws_sgd_step_scaled")


def _close(a, b, tol=1e-13):
    a, b = a.double(), b.double()
    assert a.shape == b.shape
    assert torch.equal(torch.isnan(a), torch.isnan(b))
    scale = max(float(torch.nan_to_num(b).abs().max()) if b.numel() else 0.0, 1e-300)
    assert float((torch.nan_to_num(a) - torch.nan_to_num(b)).abs().max() if b.numel() else 0.0) <= tol * scale


@pytest.mark.parametrize("lengths", [(1,), (1, 257, 64), (5, 0, 7)])
def test_segment_mean_restatement(lengths):
    g = torch.Generator().manual_seed(1)
    x = torch.rand((sum(lengths), 9), generator=g, dtype=torch.float64) * 2 - 1
    d_out = torch.rand((len(lengths), 9), generator=g, dtype=torch.float64)
    out, dx = ref.segment_mean_torch(x, lengths, d_out, torch.float64)
    _close(ref.segment_mean(x, lengths), out)
    _close(ref.segment_mean_bwd(d_out, lengths), dx)


@pytest.mark.parametrize("heads", [2, 4])
def test_max_heads_restatement_with_ties(heads):
    g = torch.Generator().manual_seed(2)
    x = torch.randint(-1, 2, (500, heads * 9), generator=g).double()          # values from {-1, 0, 1}: ties at every level
    d_out = torch.rand((500, 9), generator=g, dtype=torch.float64) + 0.5
    out, dx = ref.max_heads_torch(x, heads, d_out)
    assert torch.equal(ref.max_heads(x, heads), out)
    assert torch.equal(ref.max_heads_bwd(x, heads, d_out), dx)
    assert float((dx == 0).double().mean()) > 0.1 and int(((dx > 0) & (dx < 0.4)).sum()) > 0     # zeroed sides, halved sides


@pytest.mark.parametrize("weight", ["none", "uniform", "varied"])
def test_bce_heads_restatement(weight):
    g = torch.Generator().manual_seed(3)
    r, c, heads = 37, 9, 4
    x = (torch.rand((r, heads * c), generator=g, dtype=torch.float64) * 2 - 1) * 80
    y = torch.randint(0, 2, (r, c), generator=g).double()
    w = {"none": None, "uniform": torch.full((c,), 0.7, dtype=torch.float64),
         "varied": torch.rand(c, generator=g, dtype=torch.float64) + 0.2}[weight]
    g_heads, g_sum = torch.rand(heads, generator=g, dtype=torch.float64), 0.6
    per, total, dx = ref.bce_heads_torch(x, y, w, heads, g_heads, g_sum, torch.float64)
    per_r, total_r = ref.bce_heads(x, y, w, heads)
    _close(per_r, per)
    _close(total_r, total)
    _close(ref.bce_heads_bwd(x, y, w, heads, g_heads, g_sum), dx)


@pytest.mark.parametrize("momentum,weight_decay,max_norm", [(0.98, 1e-3, 0.05), (0.98, 0.0, 1e6), (0.0, 1e-3, 0.05)])
def test_clip_sgd_restatement(momentum, weight_decay, max_norm):
    g = torch.Generator().manual_seed(4)
    params = [torch.rand(n, generator=g, dtype=torch.float64) - 0.5 for n in (1, 3, 400, 77)]
    grads = [torch.rand(n, generator=g, dtype=torch.float64) - 0.5 for n in (1, 3, 400, 77)]
    p1, b1, g1, n1 = ref.clip_sgd(params, grads, None, 0.01, momentum, weight_decay, max_norm)
    t1 = ref.clip_sgd_torch(params, grads, 1, 0.01, momentum, weight_decay, max_norm, torch.float64)
    p2, b2, g2, n2 = ref.clip_sgd(p1, grads, b1 if momentum else None, 0.01, momentum, weight_decay, max_norm)
    t2 = ref.clip_sgd_torch(params, grads, 2, 0.01, momentum, weight_decay, max_norm, torch.float64)
    for (p, b, gr, n), t in (((p1, b1, g1, n1), t1), ((p2, b2, g2, n2), t2)):
        for mine, theirs in ((p, t[0]), (b, t[1]), (gr, t[2])):
            assert len(mine) == len(theirs)
            for a, bb in zip(mine, theirs):
                _close(a, bb, 1e-12)
        assert abs(n - float(t[3])) <= 1e-13 * n
    assert (n1 > max_norm) == (max_norm < 1)


def test_new_header_entries_parse_and_bind():
    from weasal_amd import _lib
    lib = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name][1]
    import ctypes as C
    vp = C.c_void_p
    assert _lib.SIGNATURES["ws_segment_mean_fwd"] == (C.c_int, [vp, C.c_int64, C.c_int32, C.c_int64, vp, C.c_int32, vp, vp])
    assert _lib.SIGNATURES["ws_grad_norm"] == (C.c_int, [vp, vp, C.c_int32, C.c_float, vp, C.c_int64, vp, vp])
    assert _lib.ABI.constants["WS_SGD_MAX"] == 96 and _lib.ABI.constants["WS_SGD_CHUNK"] == 4096
    assert _lib.ABI.constants["WS_SEGMENT_MAX_WIDTH"] == 1024 and _lib.ABI.constants["WS_HEADS_MAX"] == 8
    # validation needs no device: widths, sphere counts, lengths that do not sum to the rows, empty BCE input, slot counts
    one, null = vp(16), vp(None)
    lens = (C.c_int64 * 65)(*([1] * 65))
    assert lib.ws_segment_mean_fwd(one, 65, 1025, 1025, lens, 65, one, null) == 2
    assert lib.ws_segment_mean_fwd(one, 65, 4, 4, lens, 65, one, null) == 2 and b"spheres" in lib.ws_last_error()
    assert lib.ws_segment_mean_fwd(one, 60, 4, 4, lens, 64, one, null) == 1
    assert lib.ws_segment_mean_fwd(one, 64, 4, 3, lens, 64, one, null) == 1
    assert lib.ws_max_heads_fwd(one, 4, 9, 9, 81, one, null) == 2
    assert lib.ws_bce_heads_fwd(one, 0, 9, 4, 36, one, null, one, null) == 1
    sizes = (C.c_int64 * 4)(1, 0, 4096, 4097)
    assert lib.ws_grad_norm_slots(sizes, 4) == 1 + 0 + 1 + 2
    assert lib.ws_grad_norm(one, sizes, 4, 1.0, one, 3, one, null) == 1 and b"slots" in lib.ws_last_error()


class _OnDevice(torch.Tensor):
    """a CPU tensor that reports is_cuda: what the dispatch conditions see of a device tensor"""
    @property
    def is_cuda(self):
        return True


def test_switch_selects_the_old_paths(monkeypatch):
    from weasal_amd import blocks, ops
    calls = []
    monkeypatch.setattr(ops, "segment_mean", lambda x, lengths: calls.append(list(lengths)) or torch.zeros(len(lengths), x.shape[1]))
    x = torch.rand(7, 3).as_subclass(_OnDevice)
    assert blocks.WL_ENDS and blocks.wl_ends(x)
    blocks.global_average(x, np.array([3, 4], np.int32))
    blocks.global_average(x, torch.tensor([3, 4]))                              # a host tensor of lengths
    assert calls == [[3, 4], [3, 4]]
    blocks.global_average(x, torch.tensor([3, 4]).as_subclass(_OnDevice))     # lengths on the device only: the loop
    blocks.global_average(x.as_subclass(torch.Tensor).double().as_subclass(_OnDevice), [3, 4])      # float64: the loop
    blocks.global_average(torch.rand(70, 3).as_subclass(_OnDevice), [1] * 70)  # more than 64 spheres: the loop
    assert len(calls) == 2
    monkeypatch.setattr(blocks, "WL_ENDS", False)
    assert not blocks.wl_ends(x)
    out = blocks.global_average(x, [3, 4])
    assert len(calls) == 2 and out.shape == (2, 3)
    # the environment variable, in a fresh process
    code = "import sys; sys.path.insert(0, %r); from weasal_amd import blocks; print(int(blocks.WL_ENDS))" % REPO
    env = dict(os.environ, WEASAL_WL_ENDS="0")
    assert subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120).stdout.strip() == "0"


def test_cpu_tensors_never_reach_the_operators(monkeypatch):
    from weasal_amd import _lib, blocks, ops
    x = torch.rand(7, 8)
    y = (torch.rand(7, 2) > 0.5).float()
    for call in (lambda: ops.segment_mean(x, [3, 4]), lambda: ops.max_heads(x, 4),
                 lambda: ops.bce_with_logits_heads(x, y, None, 4)):
        with pytest.raises(_lib.WeasalHipError):
            call()

    def refuse(*args, **kwargs):
        raise AssertionError("a CPU tensor reached an operator of mprm_head.hip")
    for name in ("segment_mean", "max_heads", "bce_with_logits_heads"):
        monkeypatch.setattr(ops, name, refuse)
    assert blocks.WL_ENDS and not blocks.wl_ends(x)
    want = torch.stack([x[:3].mean(0), x[3:].mean(0)])
    assert torch.equal(blocks.global_average(x, [3, 4]), want)
    # the loss methods on column views of CPU tensors: criterion_multi, as before
    from weasal_amd import config as wcfg
    from weasal_amd.architectures import KPFCNN_mprm

    class Cfg(wcfg.Vaihingen3DWLConfig):
        first_features_dim = 16
    cfg = Cfg()
    np.random.seed(0)
    torch.manual_seed(0)
    net = KPFCNN_mprm(cfg, np.arange(cfg.num_classes), [])
    c = cfg.num_classes
    wide = torch.rand(3, 4 * c).requires_grad_(True)
    views = [wide[:, k * c:(k + 1) * c] for k in range(4)]
    assert ops.side_by_side(views) is not None and ops.side_by_side([v.clone() for v in views]) is None
    assert ops.side_by_side(views[::-1]) is None and ops.side_by_side(views[:3]) is None
    lb = (torch.rand(3, c) > 0.5).float()
    loss = net.class_logits_loss(views, lb)
    crit = net.criterion_multi
    want = crit(views[0], lb) + crit(views[1], lb) + crit(views[2], lb) + crit(views[3], lb) + net.reg_loss
    assert torch.equal(loss.detach(), want.detach())
    assert torch.equal(net.output_loss3.detach(), crit(views[2], lb).detach())


def test_train_step_weak_keeps_its_lines_off_the_device(monkeypatch):
    """CPU parameters (the oracle's side of the step tests) are not fusable: clip_grad_norm_ and torch's step, as before"""
    from weasal_amd import trainer
    p = torch.nn.Parameter(torch.ones(5))
    opt = trainer.FusedSGD([p], lr=0.1, momentum=0.9)
    p.grad = torch.full((5,), 2.0)
    assert not opt.fusable()
    opt.step(clip_norm=1.0)
    assert abs(float(opt.grad_norm) - 2.0 * 5 ** 0.5) < 1e-6
    assert torch.allclose(p.grad, torch.full((5,), 1 / 5 ** 0.5), atol=1e-6)
    with pytest.raises(ValueError):
        opt.step(clip_value=1.0, clip_norm=1.0)
