"""GPU: the attention kernels (weasal_amd/csrc/attention.hip) behind ops.sphere_attention / ops.channel_attention and the
attention modules of KPFCNN_mprm that call them.

Operator level.  Sphere lengths [1, 63, 64, 0, 65, 130] in ONE call: a tile edge from both sides, an empty sphere in the
middle, more than two key tiles, a single row.  Three input regimes: `mild` (Q, K uniform in +-0.5), `large` (+-2: energies of
tens, the running maximum matters), `ramp` (K rows scaled by linspace(0.1, 3, n) along the sphere: the row maximum sits in
the last key tile and the accumulated output is rescaled).  Every output and gradient is compared with tests/att_ref.py
in float64.  The bound is not a constant: per tensor and case

    max |kernel - ref64|  <=  4 * max |att_ref in float32 on the CPU - ref64|  +  1e-6 * max |ref64|

-- the float32 loop is the arithmetic the kernels replace, so the yardstick is that arithmetic, not the code under test;
4 covers one rescale rounding per key tile and the device's expf / MFMA summation order.  Each case prints its ratios.

Module level.  spatial_att, channel_att, ele_att, multi_path_att as the network builds them (tests/att_modules.py), forward
and backward, against the same classes under oracle.kpconv_ref.cpu_reference_mode: every output, input gradient and
parameter gradient within 1e-4 of the tensor's maximum (the project's fp32 contract); the same forward with torch.matmul
raising (no loop left behind the switch); the loop path in a child process with WEASAL_ATT_KERNELS=0.
A `gamma` gradient, one cancelling sum, is held to 1e-4 of the sum of its terms' magnitudes (tests/att_modules.py).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import att_modules
import att_ref

pytestmark = pytest.mark.gpu

LENGTHS = [1, 63, 64, 0, 65, 130]
N = sum(LENGTHS)
REGIMES = ("mild", "large", "ramp")
SPATIAL_WIDTHS = [(8, 64), (32, 256), (64, 512)]
CHANNEL_CASES = [(8, True), (32, True), (64, True), (64, False), (256, False)]


def _ramp(x):
    out = x.clone()
    for a, b in att_ref.spans(LENGTHS):
        if b > a:
            out[a:b] *= torch.linspace(0.1, 3.0, b - a).unsqueeze(1)
    return out


def _pair(regime, w, g):
    amp = 0.5 if regime == "mild" else 2.0
    a = (torch.rand((N, w), generator=g) * 2 - 1) * amp
    b = (torch.rand((N, w), generator=g) * 2 - 1) * amp
    return a, (_ramp(b) if regime == "ramp" else b)


@functools.lru_cache(maxsize=None)
def _spatial_case(dq, dv, regime):
    """inputs, the float64 reference and the float32 loop's error against it (computed once, shared, never modified)"""
    g = torch.Generator().manual_seed(1000 + dq + dv + REGIMES.index(regime))
    q, k = _pair(regime, dq, g)
    v = torch.rand((N, dv), generator=g) * 2 - 1
    g_att, g_xn = torch.rand((N, dv), generator=g) * 2 - 1, torch.rand((N, dv), generator=g) * 2 - 1
    r64 = att_ref.spatial_with_grads(q, k, v, LENGTHS, g_att, g_xn)
    r32 = att_ref.spatial_with_grads(q, k, v, LENGTHS, g_att, g_xn, dtype=torch.float32)
    return (q, k, v, g_att, g_xn), r64, {key: float((r32[key].double() - r64[key]).abs().max()) for key in r64}


@functools.lru_cache(maxsize=None)
def _channel_case(c, max_minus, regime):
    g = torch.Generator().manual_seed(2000 + c + 7 * int(max_minus) + REGIMES.index(regime))
    x1, x2 = _pair(regime, c, g)
    val = torch.rand((N, c), generator=g) * 2 - 1
    g_out = torch.rand((N, c), generator=g) * 2 - 1
    r64 = att_ref.channel_with_grads(x1, x2, val, LENGTHS, max_minus, g_out)
    r32 = att_ref.channel_with_grads(x1, x2, val, LENGTHS, max_minus, g_out, dtype=torch.float32)
    return (x1, x2, val, g_out), r64, {key: float((r32[key].double() - r64[key]).abs().max()) for key in r64}


def _run_spatial(gpu, inputs, grad=True):
    from weasal_amd import ops
    q, k, v, g_att, g_xn = (t.to(gpu) for t in inputs)
    q, k, v = (t.requires_grad_(grad) for t in (q, k, v))
    att, xn = ops.sphere_attention(q, k, v, LENGTHS)
    res = {"att": att.detach(), "xn": xn.detach()}
    if grad:
        ((att * g_att).sum() + (xn * g_xn).sum()).backward()
        res.update(dq=q.grad, dk=k.grad, dv=v.grad)
    return res


def _run_channel(gpu, inputs, max_minus):
    from weasal_amd import ops
    x1, x2, val, g_out = (t.to(gpu) for t in inputs)
    x1, x2, val = (t.requires_grad_(True) for t in (x1, x2, val))
    out = ops.channel_attention(x1, x2, val, LENGTHS, max_minus)
    (out * g_out).sum().backward()
    return {"out": out.detach(), "dx1": x1.grad, "dx2": x2.grad, "dvalue": val.grad}


def _check(tag, got, r64, err32):
    worst = []
    for key, ref in r64.items():
        err = float((got[key].detach().double().cpu() - ref).abs().max())
        floor = 1e-6 * float(ref.abs().max())
        bound = 4.0 * err32[key] + floor
        print("%s %-6s kernel %.3e  float32 loop %.3e  ratio %.2f  max|ref| %.3e" % (
            tag, key, err, err32[key], err / max(err32[key], 1e-300), float(ref.abs().max())))
        assert torch.isfinite(got[key]).all(), (tag, key)
        if err > bound:
            worst.append((key, err, err32[key], bound))
    assert not worst, (tag, worst)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("dq,dv", SPATIAL_WIDTHS)
def test_sphere_attention_vs_float64(gpu, dq, dv, regime):
    inputs, r64, err32 = _spatial_case(dq, dv, regime)
    _check("spatial dq=%d dv=%d %s" % (dq, dv, regime), _run_spatial(gpu, inputs), r64, err32)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("c,max_minus", CHANNEL_CASES)
def test_channel_attention_vs_float64(gpu, c, max_minus, regime):
    inputs, r64, err32 = _channel_case(c, max_minus, regime)
    _check("channel c=%d max_minus=%d %s" % (c, int(max_minus), regime), _run_channel(gpu, inputs, max_minus), r64, err32)


def test_attention_is_bit_identical_run_to_run(gpu):
    inputs, _, _ = _spatial_case(32, 256, "large")
    a, b = _run_spatial(gpu, inputs), _run_spatial(gpu, inputs)
    for key in a:
        assert torch.equal(a[key], b[key]), key
    for c, mm in ((8, True), (64, False)):
        inputs, _, _ = _channel_case(c, mm, "large")
        a, b = _run_channel(gpu, inputs, mm), _run_channel(gpu, inputs, mm)
        for key in a:
            assert torch.equal(a[key], b[key]), (c, key)


def test_forward_does_not_depend_on_requires_grad(gpu):
    for dq, dv in SPATIAL_WIDTHS:
        inputs, _, _ = _spatial_case(dq, dv, "ramp")
        with_grad, without = _run_spatial(gpu, inputs), _run_spatial(gpu, inputs, grad=False)
        assert torch.equal(with_grad["att"], without["att"]) and torch.equal(with_grad["xn"], without["xn"])


def test_strided_incoming_gradients(gpu):
    """gradients that reach the operators non-contiguous (stride-0 expansions of a sum, column slices of a wider tensor) are
    copied before the call; the copies must live until the kernels are queued: same bits as with contiguous gradients"""
    from weasal_amd import ops
    inputs, _, _ = _spatial_case(32, 256, "large")
    q, k, v, g_att, g_xn = inputs
    dv = v.shape[1]
    ones = torch.ones((N, dv))
    want = _run_spatial(gpu, (q, k, v, ones, ones))
    a, b, c = (t.to(gpu).requires_grad_(True) for t in (q, k, v))
    att, xn = ops.sphere_attention(a, b, c, LENGTHS)
    (att.sum() + xn.sum()).backward()                     # both gradients arrive expanded from one element
    for key, t in (("dq", a.grad), ("dk", b.grad), ("dv", c.grad)):
        assert torch.equal(t, want[key]), key
    want = _run_spatial(gpu, inputs)
    wide = torch.stack((g_att, g_xn), dim=2).reshape(N, 2 * dv).to(gpu)      # columns interleaved: both slices strided
    a, b, c = (t.to(gpu).requires_grad_(True) for t in (q, k, v))
    att, xn = ops.sphere_attention(a, b, c, LENGTHS)
    sa, sx = wide[:, 0::2], wide[:, 1::2]
    assert not sa.is_contiguous() and not sx.is_contiguous()
    torch.autograd.backward((att, xn), (sa, sx))
    for key, t in (("dq", a.grad), ("dk", b.grad), ("dv", c.grad)):
        assert torch.equal(t, want[key]), key
    for cc, mm in ((8, True), (64, False)):
        inputs, _, _ = _channel_case(cc, mm, "large")
        want = _run_channel(gpu, inputs, mm)
        x1, x2, val = (t.to(gpu).requires_grad_(True) for t in inputs[:3])
        wide = torch.stack((inputs[3], inputs[3] + 1), dim=2).reshape(N, 2 * cc).to(gpu)
        out = ops.channel_attention(x1, x2, val, LENGTHS, mm)
        out.backward(wide[:, 0::2])
        for key, t in (("dx1", x1.grad), ("dx2", x2.grad), ("dvalue", val.grad)):
            assert torch.equal(t, want[key]), (cc, key)


@functools.lru_cache(maxsize=None)
def _tile_height_case(c):
    """ele_att's operands as the network forms them on a Vaihingen tile: (h, h + centre height) with centre heights of
    271 m and 288.5 m through two 2 -> c projections with LeakyReLU(0.1); energies of 1e5 - 1e6, a one-hot softmax"""
    g = torch.Generator().manual_seed(3000 + c)
    h = torch.rand((N, 1), generator=g) * 3 - 1.5
    centre = torch.cat([torch.full((b - a, 1), z) for (a, b), z in zip(att_ref.spans(LENGTHS), (271.0, 288.5, 263.0, 255.0, 297.0, 280.0))])
    ele = torch.cat((h, h + centre), dim=1)
    w1, w2 = ((torch.rand((2, c), generator=g) * 2 - 1) / 2 ** 0.5 for _ in range(2))
    query, key = torch.nn.functional.leaky_relu(ele @ w1, 0.1), torch.nn.functional.leaky_relu(ele @ w2, 0.1)
    val = torch.rand((N, c), generator=g) * 2 - 1
    g_out = torch.rand((N, c), generator=g) * 2 - 1
    r64 = att_ref.channel_with_grads(query, key, val, LENGTHS, False, g_out)
    r32 = att_ref.channel_with_grads(query, key, val, LENGTHS, False, g_out, dtype=torch.float32)
    return (query, key, val, g_out), r64, {k: float((r32[k].double() - r64[k]).abs().max()) for k in r64}


@pytest.mark.parametrize("c", [64, 256])
def test_elevation_form_at_tile_heights(gpu, c):
    """the regime ele_att runs in on real tiles, held to the yardstick of the operator tests (not to a fixed 1e-4)"""
    inputs, r64, err32 = _tile_height_case(c)
    assert float(inputs[0].abs().max()) > 100.0
    _check("elevation c=%d at 255 - 297 m" % c, _run_channel(gpu, inputs, False), r64, err32)


def test_unsupported_widths(gpu):
    """dq = 12 or dv = 96: the operator raises the library's unsupported error; the module takes the loop and still matches"""
    from weasal_amd import _lib, blocks, ops
    g = torch.Generator().manual_seed(5)
    for dq, dv in ((12, 64), (8, 96)):
        q, k, v = (torch.rand((N, w), generator=g).to(gpu) for w in (dq, dq, dv))
        with pytest.raises(_lib.WeasalHipError, match="status 2"):
            ops.sphere_attention(q, k, v, LENGTHS)
    x = torch.rand((N, 6), generator=g).to(gpu)
    with pytest.raises(_lib.WeasalHipError, match="status 2"):
        ops.channel_attention(x, x, x, LENGTHS, True)
    # spatial_att at out_dim 96: dq = 12, dv = 96
    cfg = att_modules.make_config(16)
    batch, batch_cpu = _batches(gpu, 16)
    n = int(batch.points[att_modules.LAYER].shape[0])
    np.random.seed(9)
    torch.manual_seed(9)
    module = blocks.spatial_att("attention", 96, 96, cfg.first_subsampling_dl * cfg.conv_radius * 4, att_modules.LAYER, cfg)
    with torch.no_grad():
        module.gamma.fill_(0.37)
    x = torch.rand((n, 96), generator=g) * 2 - 1
    h, seeds = None, [torch.rand((n, 96), generator=g), torch.rand((n, 96), generator=g)]
    from oracle import kpconv_ref
    import copy
    with kpconv_ref.cpu_reference_mode():
        ref = att_modules.run_module("spatial_att", copy.deepcopy(module), batch_cpu, x, h, seeds)
    got = att_modules.run_module("spatial_att", copy.deepcopy(module).to(gpu), batch, x.to(gpu), h, seeds)
    _compare(got, ref, "out_dim 96")


# ---- module level -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batches(gpu, first_dim):
    return att_modules.make_batch(att_modules.make_config(first_dim), gpu)


@functools.lru_cache(maxsize=None)
def _reference(gpu, first_dim):
    return att_modules.run_all(first_dim, gpu, reference=True, batches=_batches(gpu, first_dim))


def _compare(got, ref, tag):
    assert sorted(got) == sorted(ref)
    bad = []
    for key, r in ref.items():
        if "/termsum/" in key:
            continue
        r = r.double()
        # a `gamma` gradient is one cancelling sum: 1e-4 of the sum of its terms' magnitudes (tests/att_modules.py)
        terms = ref.get(key.replace("/grad/", "/termsum/")) if r.numel() == 1 else None
        scale = r.abs().max().clamp_min(1e-30) if terms is None else terms.double().max()
        err = float((got[key].double() - r).abs().max() / scale)
        print("%s %-48s err %.3e of %s %.3e  ref %.9e got %.9e" % (tag, key, err, "max|ref|" if terms is None else "sum|terms|", float(scale),
                                                                  float(r.reshape(-1)[0]), float(got[key].reshape(-1)[0])))
        if not err < 1e-4:
            bad.append((key, err))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("first_dim", att_modules.FIRST_DIMS)
def test_modules_vs_cpu_oracle(gpu, first_dim):
    from weasal_amd import blocks
    assert blocks.ATT_KERNELS
    ref = _reference(gpu, first_dim)
    assert any(k.startswith("multi_path_att/grad/sa_f.unary1") for k in ref) and any(k.startswith("ele_att/grad/unary2") for k in ref)
    got = att_modules.run_all(first_dim, gpu, batches=_batches(gpu, first_dim))
    _compare(got, ref, "first_features_dim %d" % first_dim)


@pytest.mark.parametrize("first_dim", att_modules.FIRST_DIMS)
def test_modules_run_without_torch_matmul(gpu, first_dim, monkeypatch):
    """with the kernels on, nothing in the attention modules goes through torch.matmul (rocBLAS) any more"""
    ref = _reference(gpu, first_dim)

    def refuse(*args, **kwargs):
        raise AssertionError("torch.matmul called inside an attention module")
    monkeypatch.setattr(torch, "matmul", refuse)
    got = att_modules.run_all(first_dim, gpu, batches=_batches(gpu, first_dim), backward=False)
    monkeypatch.undo()
    _compare(got, {k: v for k, v in ref.items() if "/out" in k}, "first_features_dim %d, no torch.matmul" % first_dim)


def test_loop_path_behind_the_switch(gpu, tmp_path):
    """WEASAL_ATT_KERNELS=0 in a fresh process: the torch loop, same results within the same bound"""
    out = str(tmp_path / "loop.npz")
    env = dict(os.environ, WEASAL_ATT_KERNELS="0")
    check = ("import sys; sys.argv = ['att_modules.py', %r]; import runpy; from weasal_amd import blocks; "
             "assert not blocks.ATT_KERNELS; runpy.run_path(%r, run_name='__main__')" % (out, att_modules.__file__))
    proc = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); %s" % (att_modules.REPO, check)], env=env,
                          capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-2000:]
    arrays = np.load(out)
    for first_dim in att_modules.FIRST_DIMS:
        got = {k.split("/", 1)[1]: torch.from_numpy(arrays[k]) for k in arrays.files if k.startswith("%d/" % first_dim)}
        _compare(got, _reference(gpu, first_dim), "loop path, first_features_dim %d" % first_dim)
