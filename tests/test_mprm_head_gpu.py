"""GPU: the ends of the weak-label step as kernels (weasal_amd/csrc/mprm_head.hip, the clip-by-norm additions of optim.hip)
and their wiring into blocks.global_average, KPFCNN_mprm and trainer.train_step_weak.

Bound.  The project's rule for kernels that replace a float32 torch path (tests/test_attention_gpu.py:10-12), per tensor:

    max |kernel - ref64|  <=  4 * max |the torch float32 path on the CPU - ref64|  +  1e-6 * max |ref64|

ref64: tests/mprm_head_ref.py (pinned to torch in float64 by tests/test_mprm_head_cpu.py); the float32 path: the calls of the
reference project themselves (mprm_head_ref.*_torch at float32).  Where the issue demands bit-identity (the maximum over
heads, forward and backward; the side-by-side decoder against the per-path decoder) the comparison is torch.equal.  Every
operator is run twice and the two results compared with torch.equal.

Grid caps.  None of the new kernels caps its grid and strides: the element-wise kernels launch ceil(elements / 256)
workgroups, segment_mean one workgroup per (sphere, 64 columns), grad_sumsq / sgd_step one per 4096 elements of a tensor; the
BCE forward and the norm's finishing pass are single workgroups by design.  There is no row above a cap to run.

Run as a script (`python tests/test_mprm_head_gpu.py OUT.npz`) this file writes the small network's forward and gradients
under whatever WEASAL_WL_ENDS says: the child process of test_side_by_side_decoder_vs_per_path.
"""
import copy
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mprm_head_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64


def _held(tag, got, r64, r32):
    """the bound above for one tensor; nan must sit where the reference has it"""
    got, r64 = got.detach().double().cpu(), r64.double()
    assert got.shape == r64.shape, (tag, got.shape, r64.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(r64)), tag
    if r64.numel() == 0:
        return
    z = torch.nan_to_num
    runs32 = r32 if isinstance(r32, (list, tuple)) else [r32]       # (several evaluations of the float32 path: its largest error)
    err32 = max(float((z(t.double()) - z(r64)).abs().max()) for t in runs32)
    err, top = float((z(got) - z(r64)).abs().max()), float(z(r64).abs().max())
    print("%-58s kernel %.3e  float32 path %.3e  floor %.3e" % (tag, err, err32, 1e-6 * top))
    assert err <= 4.0 * err32 + 1e-6 * top, (tag, err, err32, top)


# ---- segment_mean ------------------------------------------------------------------------------------------------------
LENGTH_SETS = {
    "one": (1,),
    "three": (1, 257, 64),
    "sixty_four": tuple(1 + (i * 37) % 71 for i in range(64)),        # 64 spheres (the cap) of 1 to 71 rows
    "zero_inside": (5, 0, 130),
}


@functools.lru_cache(maxsize=None)
def _segment_case(name, w):
    lengths = LENGTH_SETS[name]
    g = torch.Generator().manual_seed(100 + w + len(lengths))
    x = torch.rand((sum(lengths), w), generator=g) * 2 - 1
    d_out = torch.rand((len(lengths), w), generator=g) * 2 - 1
    r64 = (ref.segment_mean(x, lengths), ref.segment_mean_bwd(d_out, lengths))
    r32 = ref.segment_mean_torch(x, lengths, d_out, F32)
    return lengths, x, d_out, r64, r32


def _run_segment(gpu, x, lengths, d_out):
    from weasal_amd import ops
    xg = x.to(gpu).requires_grad_(True)
    out = ops.segment_mean(xg, lengths)
    out.backward(d_out.to(gpu))
    return out.detach(), xg.grad


@pytest.mark.parametrize("w", [1, 9, 36, 130])
@pytest.mark.parametrize("name", sorted(LENGTH_SETS))
def test_segment_mean_vs_float64(gpu, name, w):
    lengths, x, d_out, r64, r32 = _segment_case(name, w)
    out, dx = _run_segment(gpu, x, lengths, d_out)
    _held("segment_mean %s w=%d out" % (name, w), out, r64[0], r32[0])
    _held("segment_mean %s w=%d dx" % (name, w), dx, r64[1], r32[1])
    out2, dx2 = _run_segment(gpu, x, lengths, d_out)
    assert torch.equal(out.nan_to_num(), out2.nan_to_num()) and torch.equal(dx, dx2)


def test_segment_mean_on_a_column_view(gpu):
    """W = 36 at a row stride of 40: read in place, same bits as from a contiguous copy"""
    from weasal_amd import ops
    lengths = LENGTH_SETS["three"]
    g = torch.Generator().manual_seed(7)
    base = (torch.rand((sum(lengths), 40), generator=g) * 2 - 1).to(gpu)
    view = base[:, 2:38]
    assert view.stride() == (40, 1) and not view.is_contiguous()
    d_out = torch.rand((3, 36), generator=g)
    r64 = (ref.segment_mean(view.cpu(), lengths), ref.segment_mean_bwd(d_out, lengths))
    r32 = ref.segment_mean_torch(view.cpu(), lengths, d_out, F32)
    leaf = base.clone().requires_grad_(True)
    out = ops.segment_mean(leaf[:, 2:38], lengths)
    out.backward(d_out.to(gpu))
    _held("segment_mean column view out", out, r64[0], r32[0])
    _held("segment_mean column view dx", leaf.grad[:, 2:38], r64[1], r32[1])
    assert float(leaf.grad[:, :2].abs().max()) == 0.0 and float(leaf.grad[:, 38:].abs().max()) == 0.0
    assert torch.equal(out.detach(), ops.segment_mean(view.contiguous(), lengths))
    # a gradient that arrives expanded from one element (out.sum()): copied before the call
    leaf2 = base.clone().requires_grad_(True)
    ops.segment_mean(leaf2[:, 2:38], lengths).sum().backward()
    _held("segment_mean expanded gradient", leaf2.grad[:, 2:38], ref.segment_mean_bwd(torch.ones(3, 36), lengths),
          ref.segment_mean_torch(view.cpu(), lengths, torch.ones(3, 36), F32)[1])


def test_sixty_five_spheres_take_the_loop(gpu, monkeypatch):
    from weasal_amd import _lib, blocks, ops
    lengths = [1 + i % 5 for i in range(65)]
    g = torch.Generator().manual_seed(8)
    x = torch.rand((sum(lengths), 9), generator=g) * 2 - 1
    with pytest.raises(_lib.WeasalHipError, match="status 2"):
        ops.segment_mean(x.to(gpu), lengths)
    kernel = blocks.global_average(x[:sum(lengths[:64])].to(gpu), lengths[:64])       # 64: the kernel

    def refuse(*a, **k):
        raise AssertionError("65 spheres reached ops.segment_mean")
    monkeypatch.setattr(ops, "segment_mean", refuse)
    loop = blocks.global_average(x.to(gpu), lengths)
    r64 = ref.segment_mean(x, lengths)
    r32 = ref.segment_mean_torch(x, lengths, torch.zeros(65, 9), F32)[0]
    _held("global_average, 65 spheres (loop)", loop, r64, r32)
    _held("global_average, 64 spheres (kernel)", kernel, r64[:64], r32[:64])


# ---- max_heads ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [2, 4])
@pytest.mark.parametrize("n", [1, 1000])
def test_max_heads_is_the_nested_torch_max(gpu, n, heads):
    from weasal_amd import ops
    g = torch.Generator().manual_seed(200 + n + heads)
    x = torch.rand((n, heads * 9), generator=g) * 2 - 1
    d_out = torch.rand((n, 9), generator=g) * 2 - 1
    want, want_dx = ref.max_heads_torch(x, heads, d_out)
    for _ in range(2):                                  # (run twice: bit-identical to torch, hence to itself)
        xg = x.to(gpu).requires_grad_(True)
        out = ops.max_heads(xg, heads)
        out.backward(d_out.to(gpu))
        assert torch.equal(out.detach().cpu(), want) and torch.equal(xg.grad.cpu(), want_dx)


@pytest.mark.parametrize("heads", [2, 4])
def test_max_heads_ties(gpu, heads):
    """values from {-1, 0, 1}: every tie branch of the nested backward runs"""
    from weasal_amd import ops
    g = torch.Generator().manual_seed(300 + heads)
    n, c = 1000, 9
    x = torch.randint(-1, 2, (n, heads * c), generator=g).float()
    h = [x[:, k * c:(k + 1) * c] for k in range(heads)]
    inner = h[0]
    for k in range(1, heads - 1):
        inner = torch.max(inner, h[k])
    top = torch.max(inner, h[-1])
    assert float((inner == h[-1]).float().mean()) >= 0.10               # ties in the outermost maximum
    if heads >= 3:
        assert float((sum((hk == top).float() for hk in h) >= 3).float().mean()) >= 0.01      # ties across three heads
    d_out = torch.rand((n, c), generator=g) + 0.5
    want, want_dx = ref.max_heads_torch(x, heads, d_out)
    assert torch.equal(ref.max_heads_bwd(x.double(), heads, d_out.double()).float(), want_dx)
    xg = x.to(gpu).requires_grad_(True)
    out = ops.max_heads(xg, heads)
    out.backward(d_out.to(gpu))
    assert torch.equal(out.detach().cpu(), want) and torch.equal(xg.grad.cpu(), want_dx)
    wide = torch.cat((x, x), dim=1).to(gpu)                               # a column view: row pitch 2 * heads * c
    assert torch.equal(ops.max_heads(wide[:, :heads * c], heads).cpu(), want)


# ---- BCE with logits over heads ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bce_case(r, c, heads, weight):
    g = torch.Generator().manual_seed(400 + r + heads)
    x = (torch.rand((r, heads * c), generator=g) * 2 - 1) * 80
    y = torch.randint(0, 2, (r, c), generator=g).float()
    w = {"none": None, "uniform": torch.full((c,), 0.7), "varied": torch.rand(c, generator=g) + 0.2}[weight]
    g_heads, g_sum = torch.rand(heads, generator=g), 0.6
    per64, total64 = ref.bce_heads(x, y, w, heads)
    r64 = (per64, total64, ref.bce_heads_bwd(x, y, w, heads, g_heads, g_sum))
    r32 = ref.bce_heads_torch(x, y, w, heads, g_heads, g_sum, F32)
    return x, y, w, g_heads, g_sum, r64, r32


def _run_bce(gpu, x, y, w, heads, g_heads, g_sum):
    from weasal_amd import ops
    xg = x.to(gpu).requires_grad_(True)
    per, total = ops.bce_with_logits_heads(xg, y.to(gpu), None if w is None else w.to(gpu), heads)
    ((per * g_heads.to(gpu)).sum() + total * g_sum).backward()
    return per.detach(), total.detach(), xg.grad


@pytest.mark.parametrize("weight", ["none", "uniform", "varied"])
@pytest.mark.parametrize("r,c,heads", [(1, 1, 1), (37, 9, 4), (700, 9, 4)])
def test_bce_heads_vs_float64(gpu, r, c, heads, weight):
    x, y, w, g_heads, g_sum, r64, r32 = _bce_case(r, c, heads, weight)
    assert float(x.abs().max()) > 70 or r == 1
    got = _run_bce(gpu, x, y, w, heads, g_heads, g_sum)
    for name, a, b64, b32 in zip(("per head", "sum", "dx"), got, r64, r32):
        assert torch.isfinite(a).all()
        _held("bce r=%d c=%d heads=%d %s %s" % (r, c, heads, weight, name), a, b64, b32)
    again = _run_bce(gpu, x, y, w, heads, g_heads, g_sum)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_bce_heads_gradient_of_the_sum_alone_and_empty_input(gpu):
    """loss = total (what the network's loss methods use): the per-head gradient is absent, not zeros"""
    from weasal_amd import ops
    x, y, w, g_heads, _, _, _ = _bce_case(37, 9, 4, "varied")
    xg = x.to(gpu).requires_grad_(True)
    _, total = ops.bce_with_logits_heads(xg, y.to(gpu), w.to(gpu), 4)
    total.backward()
    zero = torch.zeros(4)
    _held("bce dx of the sum alone", xg.grad, ref.bce_heads_bwd(x, y, w, 4, zero, 1.0),
          ref.bce_heads_torch(x, y, w, 4, zero, 1.0, F32)[2])
    with pytest.raises(ValueError, match="R = 0"):
        ops.bce_with_logits_heads(torch.zeros((0, 36), device=gpu), torch.zeros((0, 9), device=gpu), None, 4)


# ---- clip by norm inside the update ------------------------------------------------------------------------------------
SIZES = (1, 3, 4096, 4097, 10007, 100) + tuple(5 + (i * 7) % 60 for i in range(91))       # 97 tensors: SGD_MAX + 1
MISALIGNED = 5                                                                            # SIZES[5]: a view 4 bytes off a 16-byte line


@functools.lru_cache(maxsize=None)
def _clip_inputs():
    assert len(SIZES) == 97
    g = torch.Generator().manual_seed(500)
    params = [torch.rand(n, generator=g) - 0.5 for n in SIZES]
    grads = [torch.rand(n, generator=g) - 0.5 for n in SIZES]
    return params, grads


@functools.lru_cache(maxsize=None)
def _clip_reference(momentum, weight_decay, max_norm):
    """after the first and after the second step: ref64 and the float32 torch path"""
    params, grads = _clip_inputs()
    lr = 0.01
    a = ref.clip_sgd(params, grads, None, lr, momentum, weight_decay, max_norm)
    b = ref.clip_sgd(a[0], grads, a[1] if momentum else None, lr, momentum, weight_decay, max_norm)
    t = [ref.clip_sgd_torch(params, grads, s, lr, momentum, weight_decay, max_norm, F32) for s in (1, 2)]
    return (a, b), t


def _device_state(gpu, momentum, weight_decay):
    from weasal_amd.trainer import FusedSGD
    params, grads = _clip_inputs()
    ps = []
    for i, p in enumerate(params):
        if i == MISALIGNED:
            flat = torch.zeros(p.numel() + 8, device=gpu)
            view = flat[1:1 + p.numel()]
            view.copy_(p)
            assert view.data_ptr() % 16 == 4
            ps.append(torch.nn.Parameter(view))
        else:
            ps.append(torch.nn.Parameter(p.to(gpu)))
    gflat = torch.zeros(grads[MISALIGNED].numel() + 8, device=gpu)           # its gradient: a view of a flat buffer, as with grad_sync
    return ps, FusedSGD(ps, lr=0.01, momentum=momentum, weight_decay=weight_decay), gflat


def _device_steps(gpu, momentum, weight_decay, max_norm):
    """-> per step (params, bufs, grads, norm) on the device"""
    _, grads = _clip_inputs()
    ps, opt, gflat = _device_state(gpu, momentum, weight_decay)
    out = []
    for _ in range(2):
        for i, (p, g) in enumerate(zip(ps, grads)):
            if i == MISALIGNED:
                p.grad = gflat[3:3 + g.numel()]
                p.grad.copy_(g)
                assert p.grad.data_ptr() % 16 == 12
            else:
                p.grad = g.to(gpu)
        assert opt.fusable()
        opt.step(clip_norm=max_norm)
        bufs = [opt.state[p]["momentum_buffer"].clone() for p in ps] if momentum else []
        out.append(([p.detach().clone() for p in ps], bufs, [p.grad.clone() for p in ps], opt.grad_norm.clone()))
    return out


@pytest.mark.parametrize("max_norm", [1.0, 1000.0])                   # the gradient norm is about 39: above and below
@pytest.mark.parametrize("momentum,weight_decay", [(0.98, 1e-3), (0.98, 0.0), (0.0, 1e-3)])
def test_clip_by_norm_update_vs_float64(gpu, momentum, weight_decay, max_norm):
    (r1, r2), (t1, t2) = _clip_reference(momentum, weight_decay, max_norm)
    assert (r1[3] > max_norm) == (max_norm == 1.0)
    steps = _device_steps(gpu, momentum, weight_decay, max_norm)
    for step, (got, r64, r32) in enumerate(zip(steps, (r1, r2), (t1, t2))):
        tag = "clip m=%g wd=%g max=%g step %d" % (momentum, weight_decay, max_norm, step)
        for what, k in (("params", 0), ("bufs", 1), ("grads", 2)):
            assert len(got[k]) == len(r64[k]) == len(r32[k])
            if got[k]:
                _held("%s %s" % (tag, what), torch.cat(got[k]), torch.cat(r64[k]), torch.cat(r32[k]))
                for i in (0, 1, 3, 4, MISALIGNED, 96):                    # the odd sizes, the misaligned view and the 97th on their own
                    _held("%s %s[%d]" % (tag, what, i), got[k][i], r64[k][i], r32[k][i])
        _held("%s norm" % tag, got[3].reshape(1), torch.tensor([r64[3]], dtype=F64), r32[3].reshape(1))
    if max_norm == 1000.0:                                               # not clipped: the gradients keep their bits
        _, grads = _clip_inputs()
        assert all(torch.equal(a.cpu(), b) for a, b in zip(steps[0][2], grads))
    again = _device_steps(gpu, momentum, weight_decay, max_norm)
    for a, b in zip(steps, again):
        assert all(torch.equal(x, y) for k in range(3) for x, y in zip(a[k], b[k])) and torch.equal(a[3], b[3])


# ---- the network: side-by-side decoder, losses, whole step ------------------------------------------------------------
def _small_config():
    from weasal_amd import config as wcfg

    class Cfg(wcfg.Vaihingen3DWLConfig):
        first_features_dim = 16
    return Cfg()


def _regions_csr(region, region_lb, lens, device):
    """regions.SphereRegions from the reference's per-sphere lists (host arithmetic, one upload per tensor)"""
    from weasal_amd.regions import SphereRegions
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx, ptr, reg, sphere, lbs = [], [0], [], [], []
    for s, regs in enumerate(region):
        for r, lb in zip(regs, region_lb[s]):
            rows = np.sort(np.asarray(r, np.int64)) + off[s]
            reg.append(np.full(rows.shape[0], len(sphere), np.int32))
            idx.append(rows)
            ptr.append(ptr[-1] + rows.shape[0])
            sphere.append(s)
            lbs.append(lb)
    idx, reg, ptr = np.concatenate(idx), np.concatenate(reg), np.asarray(ptr, np.int64)
    order = np.lexsort((reg, idx))                                   # the transpose: the regions of every row, ascending
    t_ptr = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=int(off[-1])))]).astype(np.int64)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    inv_len = (1.0 / np.diff(ptr)).astype(np.float32)
    cloud_lb = np.zeros((len(lens), len(lbs[0])), np.float32)
    return SphereRegions(dev(ptr), dev(idx), dev(reg), dev(np.asarray(sphere, np.int32)), dev(np.zeros(len(sphere), np.int64)),
                         dev(np.stack(lbs).astype(np.float32)), dev(inv_len), dev(t_ptr), dev(reg[order]), dev(cloud_lb),
                         np.asarray(lens, np.int64), len(sphere), idx.shape[0])


def _small_problem(device):
    """2 spheres of 1 500 points at config 1's density, its weak labels, the network at first_features_dim 16 (CPU copy)"""
    from weasal_amd import pyramid, synthetic
    from weasal_amd.architectures import KPFCNN_mprm
    cfg = _small_config()
    wl = synthetic.WORKLOADS["vaihingen_wl"]
    pts, feats, labels, lens = synthetic.make_inputs(4242, 2, 1500, 3.2, cfg.in_features_dim)
    region, region_lb, cloud_lb, centers = synthetic.make_weak_labels(9, pts, labels, lens, num_classes=cfg.num_classes)
    centers[:, 2] = (0.8, -1.1)              # heights of about a metre: float32 carries 1e-4 there (tests/att_modules.py)
    assert all(len(r) > 0 for r in region)
    np.random.seed(31)
    batch = pyramid.build_batch(cfg, torch.from_numpy(pts).to(device), torch.from_numpy(feats).to(device),
                                torch.from_numpy(labels).to(device), lens, wl["limits"])
    batch.center_pts = torch.from_numpy(centers).to(device)
    batch.cloud_lb = torch.from_numpy(cloud_lb).to(device)
    np.random.seed(5)
    torch.manual_seed(5)
    net = KPFCNN_mprm(cfg, np.arange(cfg.num_classes), [])
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("gamma"):
                p.fill_(0.37)
    return cfg, batch, net, (region, region_lb, cloud_lb, centers, lens)


def _forward_and_gradients(cfg, batch, net, weak, device):
    """forward, class_logits_loss + region_mprm_loss over the device regions, backward -> {name: CPU tensor}"""
    region, region_lb, _, _, lens = weak
    net = copy.deepcopy(net).to(device).train()
    logits, cla, cam = net(batch, cfg)
    loss = net.class_logits_loss(cla, batch.cloud_lb) + net.region_mprm_loss(cam, _regions_csr(region, region_lb, lens, device), None, None)
    loss.backward()
    res = {"logits": logits, "loss": loss.reshape(1)}
    res.update({"cam%d" % i: t for i, t in enumerate(cam)})
    res.update({"cla%d" % i: t for i, t in enumerate(cla)})
    res.update({"grad/" + n: p.grad for n, p in net.named_parameters() if p.grad is not None})
    return {k: v.detach().cpu().clone() for k, v in res.items()}


def _oracle(cfg, batch, net, weak, dtype):
    """the same classes under oracle.kpconv_ref.cpu_reference_mode at `dtype`; the region loss as the reference writes it
    (architectures.py:752-783: mean of every region's rows, criterion_multi per path)"""
    from oracle import kpconv_ref
    from weasal_amd.pyramid import PyramidBatch
    region, region_lb, cloud_lb, centers, lens = weak
    cast = lambda t: t.detach().cpu().to(dtype) if t.is_floating_point() else t.detach().cpu()
    flat = batch.points + batch.neighbors + batch.pools + batch.upsamples + batch.lengths + [batch.features, batch.labels]
    b = PyramidBatch([cast(t) for t in flat])
    b.center_pts = torch.from_numpy(centers).to(dtype)
    net = copy.deepcopy(net).to(dtype).train()
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    with kpconv_ref.cpu_reference_mode():
        logits, cla, cam = net(b, cfg)
        loss = net.class_logits_loss(cla, torch.from_numpy(cloud_lb).to(dtype))
        lbs = torch.from_numpy(np.stack([lb for s in region_lb for lb in s])).to(dtype)
        for k in range(4):
            means = torch.stack([cam[k][torch.from_numpy(np.asarray(r, np.int64) + off[s])].mean(dim=0)
                                 for s, regs in enumerate(region) for r in regs])
            loss = loss + net.criterion_multi(means, lbs)
        loss.backward()
    res = {"logits": logits, "loss": loss.reshape(1)}
    res.update({"cam%d" % i: t for i, t in enumerate(cam)})
    res.update({"cla%d" % i: t for i, t in enumerate(cla)})
    res.update({"grad/" + n: p.grad for n, p in net.named_parameters() if p.grad is not None})
    return {k: v.detach().clone() for k, v in res.items()}


def test_side_by_side_decoder_vs_per_path(gpu, tmp_path):
    """WEASAL_WL_ENDS = 1 (this process) and 0 (a fresh one): logits and CAMs bit-identical; class logits, loss and every
    parameter gradient held to the float64 oracle by the bound at the head of this file.
    The float32 path here is the whole network on the CPU oracle, and its threaded sums do not add in one order on every
    host (tests/att_modules.py): for the most cancelling gradient, ele_head.unary2, ONE evaluation erred by 2.1e-8 on one
    host and by 4.6e-9 on another (the kernels: 2.1e-8).  It is therefore evaluated twice, with torch's threads and with
    one thread -- two summation orders of the same calls -- and its error is the larger of the two."""
    from weasal_amd import blocks, ops
    assert blocks.WL_ENDS
    cfg, batch, net, weak = _small_problem(gpu)
    assert 2500 < int(batch.points[0].shape[0]) <= 3000
    on = _forward_and_gradients(cfg, batch, net, weak, gpu)
    out = str(tmp_path / "off.npz")
    proc = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, WEASAL_WL_ENDS="0"),
                          capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    off = {k: torch.from_numpy(v) for k, v in np.load(out).items()}
    assert sorted(on) == sorted(off)
    for key in ["logits"] + ["cam%d" % i for i in range(4)]:
        assert torch.equal(on[key], off[key]), key
    r64, r32 = _oracle(cfg, batch, net, weak, F64), _oracle(cfg, batch, net, weak, F32)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        r32_one = _oracle(cfg, batch, net, weak, F32)
    finally:
        torch.set_num_threads(threads)
    assert sorted(r64) == sorted(on)
    for key in sorted(on):
        _held("WL_ENDS=1 " + key, on[key], r64[key], [r32[key], r32_one[key]])
    # the wide tensors are what the loss methods saw: the four CAMs are column views of one base
    net_g = copy.deepcopy(net).to(gpu)
    _, cla, cam = net_g(batch, cfg)
    assert ops.side_by_side(cam) is not None and ops.side_by_side(cla) is not None


def test_whole_step_vs_oracle(gpu):
    """train_step_weak with the switch on -- device regions, so the region means, the BCE heads and the clip-by-norm update
    all run as kernels -- against the same classes on the CPU oracle, at the bounds of
    test_weak_label_gpu.py::test_config1_real_shape_step_vs_oracle: logits, class logits and CAMs 1e-4, loss 1e-5, gradient
    norm 1e-3, parameters after the step 1e-4"""
    from oracle import kpconv_ref
    from test_fullwidth_gpu import _cpu_copy
    from weasal_amd import blocks
    from weasal_amd.trainer import FusedSGD, make_optimizer, train_step_weak
    assert blocks.WL_ENDS
    cfg, batch, net, weak = _small_problem(gpu)
    region, region_lb, cloud_lb, centers, lens = weak
    cfg.grad_clip_norm = 0.02                      # below the gradient norm: the scaling branch
    net_cpu = copy.deepcopy(net).train()
    net = net.to(gpu).train()
    opt = make_optimizer(net, cfg)
    batch.region, batch.region_lb = _regions_csr(region, region_lb, lens, gpu), None
    calls = []
    real = FusedSGD.step
    FusedSGD.step = lambda self, *a, **k: calls.append(k) or real(self, *a, **k)
    try:
        loss, (logits, cla, cam) = train_step_weak(net, opt, batch, cfg)
    finally:
        FusedSGD.step = real
    assert calls == [{"clip_norm": 0.02}] and net.grad_norm.is_cuda and net.grad_norm.dim() == 0
    batch_cpu = _cpu_copy(batch)
    batch_cpu.region, batch_cpu.region_lb = region, region_lb
    batch_cpu.cloud_lb, batch_cpu.center_pts = torch.from_numpy(cloud_lb), torch.from_numpy(centers)
    opt_c = make_optimizer(net_cpu, cfg)
    with kpconv_ref.cpu_reference_mode():
        loss_c, (logits_c, cla_c, cam_c) = train_step_weak(net_cpu, opt_c, batch_cpu, cfg)
    assert float(net_cpu.grad_norm) > cfg.grad_clip_norm
    rel = lambda a, b: float((a.detach().double().cpu() - b.detach().double()).abs().max() / b.detach().double().abs().max().clamp_min(1e-30))
    assert rel(logits, logits_c) < 1e-4
    for a, b in zip(list(cla) + list(cam), list(cla_c) + list(cam_c)):
        assert rel(a, b) < 1e-4
    print("loss %.9e oracle %.9e  norm %.6e oracle %.6e" % (float(loss), float(loss_c), float(net.grad_norm), float(net_cpu.grad_norm)))
    assert abs(float(loss) - float(loss_c)) <= 1e-5 * abs(float(loss_c))
    assert abs(float(net.grad_norm) - float(net_cpu.grad_norm)) <= 1e-3 * float(net_cpu.grad_norm)
    ref_p = dict(net_cpu.named_parameters())
    for name, p in net.named_parameters():
        assert rel(p, ref_p[name]) < 1e-4, name


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    cfg_, batch_, net_, weak_ = _small_problem(dev)
    np.savez(sys.argv[1], **{k: v.numpy() for k, v in _forward_and_gradients(cfg_, batch_, net_, weak_, dev).items()})
