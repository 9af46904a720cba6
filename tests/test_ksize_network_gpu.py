"""GPU: whole networks with 9 and 13 kernel points -- config.num_kernel_points is all a user sets.

Two small KP-FCNNs (at most 64 channels wide, 2 spheres of 3 000 points, the batch from pyramid.build_batch), one training
step each on the GPU against the CPU oracle (oracle.kpconv_ref.cpu_reference_mode: the reference's op sequence in plain
torch) on the SAME index matrices and the same initial state:
  * rigid, num_kernel_points = 13: every block through the block calls (ws_kpblock_fwd / _bwd) -- K3 / K4 / K4G at K = 13;
  * deformable + modulated, f32 rows, num_kernel_points = 9: the generic MODE 1 + DEF route (the packed fast path is K = 15
    only), K6, the regulariser kernels at K = 9.
Tolerances: those of the golden network step (tests/test_pyramid_gpu.py::test_kpfcnn_step_vs_golden) -- logits 1e-4 of
max|ref|, loss 1e-5, every parameter gradient 1e-3 of its maximum, parameters after the step 1e-4.
The state dict carries K: weights [K, Ci, Co], offset_dim = (p_dim + 1) K.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# two levels, 32 and 64 channels wide.  (Not narrower: with 4 096 rows or more and an output of 8 channels or fewer the shallow
# dense product asks for more LDS than a workgroup has, at any kernel size -- the contraction of a 16-wide first layer.)
_ARCH = ['simple', 'resnetb', 'resnetb_strided', 'resnetb', 'nearest_upsample', 'unary']


def make_config(k, deformable):
    from weasal_amd.config import Config

    class Cfg(Config):
        architecture = [b.replace('resnetb', 'resnetb_deformable') if (deformable and i >= 2) else b for i, b in enumerate(_ARCH)]
        num_kernel_points = k
        first_subsampling_dl = 0.24
        deform_radius = 5.0 if deformable else 6.0
        modulated = deformable
        first_features_dim = 32
        in_features_dim = 4
        batch_norm_momentum = 0.02
        repulse_extent = 1.2
        learning_rate = 0.01
        momentum = 0.98
        dropout = 0
        saving = False
    return Cfg()


def rel(a, b):
    a = np.asarray(a.detach().cpu().numpy(), np.float64)
    b = np.asarray(b.detach().cpu().numpy(), np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _cpu_copy(batch):
    from weasal_amd.pyramid import PyramidBatch
    flat = batch.points + batch.neighbors + batch.pools + batch.upsamples + batch.lengths + [batch.features, batch.labels]
    return PyramidBatch([t.detach().cpu() for t in flat])


def _step_vs_oracle(gpu, cfg, limits):
    from oracle import kpconv_ref
    from weasal_amd import pyramid, synthetic
    from weasal_amd.architectures import KPFCNN
    from weasal_amd.trainer import make_optimizer, train_step
    k = cfg.num_kernel_points
    np.random.seed(4)
    torch.manual_seed(4)
    net_cpu = KPFCNN(cfg, np.arange(9), []).train()
    for name, p in net_cpu.state_dict().items():
        if name.endswith("KPConv.weights") or name.endswith("offset_conv.weights"):
            assert p.shape[0] == k, (name, tuple(p.shape))
        if name.endswith("offset_bias"):
            assert p.shape[0] == 4 * k, (name, tuple(p.shape))          # (p_dim + 1) K: modulated
    widest = max(p.shape[-1] for n, p in net_cpu.state_dict().items() if n.endswith("weights"))
    assert widest <= 64, widest
    np.random.seed(4)
    net = KPFCNN(cfg, np.arange(9), [])
    net.load_state_dict(net_cpu.state_dict())
    net.to(gpu).train()
    pts, feats, labels, lens = synthetic.make_inputs(31, 2, 3000, 3.0, cfg.in_features_dim)
    np.random.seed(8)
    batch = pyramid.build_batch(cfg, torch.from_numpy(pts).to(gpu), torch.from_numpy(feats).to(gpu),
                                torch.from_numpy(labels).to(gpu), lens, limits)
    bc = _cpu_copy(batch)
    opt = make_optimizer(net, cfg)
    loss, out = train_step(net, opt, batch, cfg)
    torch.cuda.synchronize()
    # the oracle: the same step on the CPU
    opt_c = make_optimizer(net_cpu, cfg)
    opt_c.zero_grad()
    with kpconv_ref.cpu_reference_mode():
        out_c = net_cpu(bc, cfg)
        loss_c = net_cpu.loss(out_c, bc.labels)
        loss_c.backward()
    grads_c = {n: p.grad.clone() for n, p in net_cpu.named_parameters() if p.grad is not None}
    torch.nn.utils.clip_grad_value_(net_cpu.parameters(), cfg.grad_clip_norm)
    opt_c.step()
    figures = {"logits": rel(out, out_c), "loss": abs(loss.item() - loss_c.item())}
    params = dict(net.named_parameters())
    gerr = {n: rel(params[n].grad, g) for n, g in grads_c.items()}
    perr = {n: rel(p, net_cpu.state_dict()[n]) for n, p in net.state_dict().items() if p.is_floating_point()}
    figures["worst grad"] = max(gerr.items(), key=lambda kv: kv[1])
    figures["worst param"] = max(perr.items(), key=lambda kv: kv[1])
    print("FIGURES K=%d" % k, figures)
    assert all((params[n].grad is None) == (n not in grads_c) for n in params)
    assert figures["logits"] < 1e-4
    assert figures["loss"] < 1e-5
    for n, e in gerr.items():
        assert e < 1e-3, (n, e)
    for n, e in perr.items():
        assert e < 1e-4, (n, e)
    return net


def test_rigid_network_k13_step_vs_oracle(gpu):
    from weasal_amd import fused
    calls = {"kp": 0}
    kp_apply = fused._KPBlockFn.apply

    def kp(*a):
        calls["kp"] += 1
        return kp_apply(*a)
    fused._KPBlockFn.apply = kp
    try:
        _step_vs_oracle(gpu, make_config(13, False), [30, 35])
    finally:
        fused._KPBlockFn.apply = kp_apply
    assert calls["kp"] == 4, calls          # every KPConv block of the encoder ran as one block call


def test_deformable_modulated_network_k9_step_vs_oracle(gpu):
    from weasal_amd import architectures
    seen = []
    reg = architectures.ops.p2p_regularizer

    def spy(*a, **kw):
        seen.append(tuple(a[0].shape))
        return reg(*a, **kw)
    architectures.ops.p2p_regularizer = spy
    try:
        net = _step_vs_oracle(gpu, make_config(9, True), [60, 60])
    finally:
        architectures.ops.p2p_regularizer = reg
    layers = [m for m in net.modules() if getattr(m, "deformable", False)]
    assert len(layers) == 2 and all(m.K == 9 and m.offset_dim == 36 for m in layers)
    assert len(seen) == 2 and all(s[1:] == (9, 3) for s in seen)          # the regulariser kernels ran at K = 9
