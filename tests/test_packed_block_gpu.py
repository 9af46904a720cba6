"""The strided blocks of the training step with the packed table walk of K4 (ws_block_packed_k4 = 1, the default) and
without it (= 0, the launch sequence before it): the same step bit for bit -- logits, loss and every parameter gradient
torch.equal -- behind the same number of launches.  The step is the small one of tests/test_fused_blocks_gpu.py (3 x 4 000
points, limits [40, 45, 50, 50, 40], every block through the block calls)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PACKED = "kpconv_gather_bwd_x_packed_kernel"


def _step(gpu, cfg):
    """(logits, loss, gradients, launches, [(nq, ns, h, ci) of the strided blocks])"""
    from weasal_amd import _lib, fused, pyramid, synthetic
    from weasal_amd.architectures import KPFCNN
    from weasal_amd.blocks import KPConv
    from weasal_amd.trainer import make_optimizer, train_step
    lib = _lib.lib()
    min_rows, fused.MIN_ROWS = fused.MIN_ROWS, 0
    try:
        np.random.seed(3)
        torch.manual_seed(3)
        net = KPFCNN(cfg, np.arange(9), []).to(gpu).train()
        opt = make_optimizer(net, cfg)
        pts, feats, labels, lens = synthetic.make_inputs(21, 3, 4000, 4.0, cfg.in_features_dim)
        np.random.seed(8)
        batch = pyramid.build_batch(cfg, torch.from_numpy(pts).to(gpu), torch.from_numpy(feats).to(gpu),
                                    torch.from_numpy(labels).to(gpu), lens, [40, 45, 50, 50, 40])
        n0 = lib.ws_launch_count()
        loss, out = train_step(net, opt, batch, cfg)
        torch.cuda.synchronize()
        launches = lib.ws_launch_count() - n0
        grads = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
        widths = [[c for c in m.modules() if isinstance(c, KPConv)][0].in_channels
                  for m in net.modules() if "strided" in getattr(m, "block_name", "")]
        shapes = [(batch.points[l + 1].shape[0], batch.points[l].shape[0], batch.pools[l].shape[1], ci) for l, ci in enumerate(widths)]
        return out.detach().clone(), loss.item(), grads, launches, shapes
    finally:
        fused.MIN_ROWS = min_rows


def test_step_is_unchanged_by_the_packed_walk(gpu):
    from weasal_amd import _lib, config as wcfg, fused, ops
    lib = fused._bind()
    switch = C.c_int.in_dll(lib, "ws_block_packed_k4")
    cfg = wcfg.DALESPLConfig()
    cfg.dropout = 0.0
    before = switch.value
    try:
        switch.value = 0
        out0, loss0, g0, n_0, shapes = _step(gpu, cfg)
        switch.value = 1
        out1, loss1, g1, n_1, _ = _step(gpu, cfg)
    finally:
        switch.value = before
    assert torch.equal(out0, out1) and loss0 == loss1
    assert set(g0) == set(g1) and len(g0) > 30
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    assert n_0 == n_1 and n_0 > 0
    # at least one strided block took the packed kernel: the reporter at the blocks' shapes
    assert len(shapes) >= 3, shapes
    took = []
    for nq, ns, h, ci in shapes:
        buf = C.create_string_buffer(256)
        _lib.check(lib.ws_kpconv_gather_bwd_x_packed_variant(nq, ns, h, ci, 0x10000000, 0x20000000, 0, 0, ops.INFLUENCE["linear"],
                                                             ops.AGGREGATION["sum"], 0, 1, buf, 256))
        took.append(buf.value.decode().startswith(PACKED))
    assert any(took), shapes
