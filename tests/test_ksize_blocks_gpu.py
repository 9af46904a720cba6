"""GPU: whole blocks and their dense products at the kernel sizes other than 15.

* ws_kpblock_fwd / _bwd (weasal_amd/fused.py) with 13 kernel points: the DALES network -- `simple`, `resnetb` and
  `resnetb_strided` blocks at every level -- through the block calls against the operator-by-operator path of
  weasal_amd/blocks.py, one training step on the same inputs, at the bounds tests/test_fused_blocks_gpu.py holds the K = 15
  network to (same harness: its _run).  The block calls are counted: none may fall back.
* The kernel contraction has depth K Ci: 9 x 32 and 13 x 64 in the body of a network, 9, 13, 36 (9 x 4) and 52 (13 x 4) at the
  input layer.  Forward (ws_gemm_xb_epilogue_strided: wf [M, K Ci] . W) and weight gradient (ws_gemm_xty: wf^T . dy) at those
  depths, on a level above and below 4 096 rows, held per element to float64 by the harness and bound of
  tests/test_gemm_branches_gpu.py (its run_xb / run_xty, which also make the library's reporter name the plan stated here):
  every depth goes through a branch the products already have -- no kernel was added for them.
"""
import pytest
import torch

import test_fused_blocks_gpu as FB
import test_gemm_branches_gpu as GM

pytestmark = pytest.mark.gpu


def test_block_calls_match_operator_path_k13(gpu):
    from weasal_amd import config as wcfg, fused
    cfg = wcfg.DALESPLConfig()
    cfg.dropout = 0.0
    cfg.num_kernel_points = 13
    calls = {"kp": 0}
    kp_apply = fused._KPBlockFn.apply

    def kp(*a):
        calls["kp"] += 1
        return kp_apply(*a)
    fused._KPBlockFn.apply = kp
    try:
        out_f, loss_f, g_f, p_f = FB._run(gpu, cfg, True)
    finally:
        fused._KPBlockFn.apply = kp_apply
    assert calls["kp"] == 10, calls                     # simple + 5 resnetb + 4 resnetb_strided, as at K = 15
    assert p_f["encoder_blocks.0.KPConv.weights"].shape[0] == 13
    out_o, loss_o, g_o, p_o = FB._run(gpu, cfg, False)
    assert FB.rel(out_f, out_o) < 2e-5
    assert abs(loss_f - loss_o) < 1e-5 * abs(loss_o)
    assert set(g_f) == set(g_o) and len(g_f) > 30
    num = sum(float(((g_f[k].double() - g_o[k].double()) ** 2).sum()) for k in g_o)
    den = sum(float((g_o[k].double() ** 2).sum()) for k in g_o)
    print("FIGURES out %.3g loss %.3g grad vector %.3g" % (FB.rel(out_f, out_o), abs(loss_f - loss_o) / abs(loss_o), (num / den) ** 0.5))
    assert (num / den) ** 0.5 < 5e-4
    for k in g_o:
        assert FB.rel(g_f[k], g_o[k]) < 5e-2, k
    for k in p_o:
        assert FB.rel(p_f[k], p_o[k]) < 2e-5, k


def test_block_inference_k13_matches_training_forward(gpu):
    """under no_grad a 32 -> 32 block of the K = 15 network runs the one-launch forward layer; at K = 13 the same block call
    takes gather + contraction (the fused layer is K = 15 only) and returns the training forward's values"""
    import numpy as np
    from weasal_amd import config as wcfg, pyramid, synthetic
    from weasal_amd.architectures import KPFCNN
    cfg = wcfg.DALESPLConfig()
    cfg.dropout = 0.0
    cfg.num_kernel_points = 13
    np.random.seed(3)
    torch.manual_seed(3)
    net = KPFCNN(cfg, np.arange(9), []).to(gpu).eval()
    pts, feats, labels, lens = synthetic.make_inputs(21, 2, 3000, 4.0, cfg.in_features_dim)
    np.random.seed(8)
    batch = pyramid.build_batch(cfg, torch.from_numpy(pts).to(gpu), torch.from_numpy(feats).to(gpu), torch.from_numpy(labels).to(gpu),
                                lens, [40, 45, 50, 50, 40])
    with torch.no_grad():
        a = net(batch, cfg)
    b = net(batch, cfg)
    assert torch.isfinite(a).all() and FB.rel(a, b) < 2e-5


_T2 = "gemm_xty2_kernel<KT=%d, NT=%d, WK=%d, WN=1, TI=float> chunk=%d chunks=%d reduce=reduce_partials_kernel out=flat"
# (rows, depth K Ci, Co, forward plan, dW plan)
DEPTHS = [
    (600, 288, 32, GM._x2(1, 1, csplit=9), _T2 % (2, 1, 2, 64, 10)),
    (600, 832, 64, GM._x2(1, 2, splits=3, csplit=9), _T2 % (2, 2, 2, 64, 10)),
    (600, 9, 32, GM._xg(1, 0, 1), _T2 % (1, 1, 1, 64, 10)),
    (600, 13, 32, GM._xg(1, 0, 1), _T2 % (1, 1, 1, 64, 10)),
    (600, 36, 32, GM._xg(1, 1, 1), _T2 % (2, 1, 1, 64, 10)),
    (600, 52, 64, GM._xg(2, 1, 1), _T2 % (2, 2, 1, 64, 10)),
    (5000, 288, 32, GM._x2(1, 1, csplit=9), _T2 % (2, 1, 2, 64, 79)),
    (5000, 832, 64, GM._x2(1, 2, splits=3, csplit=9), _T2 % (2, 2, 2, 160, 32)),
    (5000, 9, 32, GM._sh(256), _T2 % (1, 1, 1, 64, 79)),
    (5000, 13, 32, GM._sh(256), _T2 % (1, 1, 1, 64, 79)),
    (5000, 36, 32, GM._sh(256), _T2 % (2, 1, 1, 64, 79)),
    (5000, 52, 64, GM._sh(128), _T2 % (2, 2, 1, 64, 79)),
]


@pytest.mark.parametrize("m,k,n,fwd,dw", DEPTHS, ids=["m%d-k%d-n%d" % d[:3] for d in DEPTHS])
def test_contraction_depths_vs_float64(m, k, n, fwd, dw):
    with GM.Flag("ws_gemm_shallow", 1), GM.Flag("ws_gemm_staged", 1):
        w1 = GM.run_xb(GM._xb("ksize_xb_m%d_k%d_n%d" % (m, k, n), fwd, m, k, n, scratch=GM.FULL))
        w2 = GM.run_xty(GM._xty("ksize_xty_m%d_k%d_n%d" % (m, k, n), dw, m, k, n))
    print("FIGURES worst |err| / bound: forward %.3g, dW %.3g" % (w1, w2))
