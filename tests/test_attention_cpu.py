"""CPU (no GPU needed): the attention entries of the C ABI and the float32 yardstick of the attention tests.

  * tests/att_ref.py in float32 is the arithmetic of the module loops of weasal_amd/blocks.py (spatial_att, channel_att,
    ele_att) on CPU tensors: same values at 1e-6;
  * include/weasal_hip.h declares the four attention entries and the built library exports them;
  * the entries validate on the host, with no device: sum(lengths) != N, a negative length and a NULL pointer are
    WS_ERR_INVALID, an unsupported width or too many spheres WS_ERR_UNSUPPORTED.
"""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import att_ref
from conftest import REPO

ENTRIES = ("ws_sphere_attention_fwd", "ws_sphere_attention_bwd", "ws_channel_attention_fwd", "ws_channel_attention_bwd")
LENGTHS = [5, 17, 0, 9]


def _identity_module(cls, first_dim):
    """the attention module with its projections replaced by fixed row-wise maps, so that its loop can be fed directly"""
    from weasal_amd import config as wcfg

    class Cfg(wcfg.Vaihingen3DWLConfig):
        first_features_dim = first_dim
    return cls("att", first_dim, first_dim, 1.0, 0, Cfg())


class _Pass(torch.nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x, batch=None):
        return self.fn(x)


def _batch(n):
    return types.SimpleNamespace(lengths_host=[LENGTHS], lengths=[torch.tensor(LENGTHS)],
                                 center_pts=torch.zeros((len(LENGTHS), 3)))


def test_att_ref_float32_is_the_module_loop():
    from weasal_amd import blocks
    g = torch.Generator().manual_seed(3)
    n, d = sum(LENGTHS), 64
    feats = torch.rand((n, d), generator=g) - 0.5
    wq, wk = torch.rand((d, d // 8), generator=g) - 0.5, torch.rand((d, d // 8), generator=g) - 0.5
    wv = torch.rand((d, d), generator=g) - 0.5
    batch = _batch(n)
    ident = _Pass(lambda x: x)

    m = _identity_module(blocks.spatial_att, d)
    m.simple1, m.simple2 = ident, ident
    m.unary1, m.unary2, m.unary3 = _Pass(lambda x: x @ wq), _Pass(lambda x: x @ wk), _Pass(lambda x: x @ wv)
    with torch.no_grad():
        m.gamma.fill_(1.0)
        merged, xn = m(feats, batch)
    att, xn_ref = att_ref.spatial(feats @ wq, feats @ wk, feats @ wv, LENGTHS)
    assert torch.allclose(merged - feats, att, rtol=0, atol=1e-6) and torch.allclose(xn, xn_ref, rtol=0, atol=1e-6)

    m = _identity_module(blocks.channel_att, d)
    m.simple1, m.simple2 = ident, ident
    w1, w2 = torch.rand((d, d), generator=g) - 0.5, torch.rand((d, d), generator=g) - 0.5
    m.unary1, m.unary2 = _Pass(lambda x: x @ w1), _Pass(lambda x: x @ w2)
    with torch.no_grad():
        m.gamma.fill_(1.0)
        merged = m(feats, batch)
    out = att_ref.channel(feats @ w1, feats @ w2, feats, LENGTHS, True)
    assert torch.allclose(merged - feats, out, rtol=0, atol=1e-6)

    m = _identity_module(blocks.ele_att, d)
    m.simple2 = ident
    h = torch.rand((n, 1), generator=g)
    e1, e2 = torch.rand((2, d), generator=g) - 0.5, torch.rand((2, d), generator=g) - 0.5
    m.unary1, m.unary2 = _Pass(lambda x: x @ e1), _Pass(lambda x: x @ e2)
    with torch.no_grad():
        m.gamma.fill_(1.0)
        merged = m(feats, h, batch)
    ele = torch.cat((h, h), dim=1)                         # centre heights are zero in this batch
    out = att_ref.channel(ele @ e1, ele @ e2, feats, LENGTHS, False)
    assert torch.allclose(merged - feats, out, rtol=0, atol=1e-6)


def test_att_ref_float32_tracks_float64():
    g = torch.Generator().manual_seed(5)
    n = sum(LENGTHS)
    q, k, v = (torch.rand((n, w), generator=g) - 0.5 for w in (8, 8, 64))
    ga, gx = torch.rand((n, 64), generator=g), torch.rand((n, 64), generator=g)
    r64 = att_ref.spatial_with_grads(q, k, v, LENGTHS, ga, gx)
    r32 = att_ref.spatial_with_grads(q, k, v, LENGTHS, ga, gx, dtype=torch.float32)
    for key in r64:
        assert r32[key].dtype == torch.float32 and r64[key].dtype == torch.float64
        assert float((r32[key].double() - r64[key]).abs().max()) <= 1e-5 * float(r64[key].abs().max())


def test_header_declares_and_library_exports_the_attention_entries():
    from weasal_amd import _lib
    text = open(os.path.join(REPO, "include", "weasal_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ws_[a-z0-9_]+)\s*\(", text))
    lib = _lib.lib()
    for name in ENTRIES:
        assert name in declared, "include/weasal_hip.h does not declare %s" % name
        assert hasattr(lib, name), "libweasal_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES


def test_attention_argument_validation_needs_no_device():
    from weasal_amd import _lib
    lib = _lib.lib()
    null = C.c_void_p(None)
    one = C.c_void_p(16)                                   # never dereferenced: validation fails first
    lens = lambda *v: (C.c_int64 * len(v))(*v)
    INVALID, UNSUPPORTED = 1, 2

    def sfwd(n, dq, dv, lengths, ns, q=one):
        return lib.ws_sphere_attention_fwd(q, one, one, n, dq, dv, lengths, ns, one, one, null, null)

    def sbwd(n, dq, dv, lengths, ns, d_att=one, scratch=one):
        return lib.ws_sphere_attention_bwd(one, one, one, one, one, d_att, null, n, dq, dv, lengths, ns, one, one, one, scratch, 1 << 40,
                                           null)

    def cfwd(n, c, lengths, ns, x1=one):
        return lib.ws_channel_attention_fwd(x1, one, one, n, c, lengths, ns, 1, one, one, one, 1 << 40, null)

    def cbwd(n, c, lengths, ns, d_out=one):
        return lib.ws_channel_attention_bwd(one, one, one, one, d_out, n, c, lengths, ns, 0, one, one, one, one, 1 << 40, null)

    # sum(lengths) != N
    for rc in (sfwd(10, 8, 64, lens(4, 5), 2), sbwd(10, 8, 64, lens(4, 5), 2), cfwd(10, 8, lens(4, 7), 2), cbwd(10, 8, lens(4, 7), 2)):
        assert rc == INVALID and b"sum" in lib.ws_last_error()
    # a negative length
    for rc in (sfwd(10, 8, 64, lens(12, -2), 2), sbwd(10, 8, 64, lens(12, -2), 2), cfwd(10, 8, lens(12, -2), 2),
               cbwd(10, 8, lens(12, -2), 2)):
        assert rc == INVALID and b"negative" in lib.ws_last_error()
    # NULL pointers: an operand, the length vector, the incoming gradient, the scratch
    assert sfwd(10, 8, 64, lens(4, 6), 2, q=null) == INVALID and b"NULL" in lib.ws_last_error()
    assert sfwd(10, 8, 64, null, 2) == INVALID
    assert sbwd(10, 8, 64, lens(4, 6), 2, d_att=null) == INVALID
    assert sbwd(10, 8, 64, lens(4, 6), 2, scratch=null) == INVALID
    assert cfwd(10, 8, lens(4, 6), 2, x1=null) == INVALID and b"NULL" in lib.ws_last_error()
    assert cbwd(10, 8, lens(4, 6), 2, d_out=null) == INVALID
    assert cfwd(10, 8, null, 2) == INVALID
    # widths the kernels do not take, more spheres than the kernel arguments carry
    assert sfwd(10, 12, 64, lens(10), 1) == UNSUPPORTED and b"dq" in lib.ws_last_error()
    assert sfwd(10, 8, 96, lens(10), 1) == UNSUPPORTED
    assert sfwd(10, 68, 64, lens(10), 1) == UNSUPPORTED and sfwd(10, 8, 576, lens(10), 1) == UNSUPPORTED
    assert cfwd(10, 6, lens(10), 1) == UNSUPPORTED and cfwd(10, 516, lens(10), 1) == UNSUPPORTED
    many = lens(*([1] * 65))
    assert sfwd(65, 8, 64, many, 65) == UNSUPPORTED and cfwd(65, 8, many, 65) == UNSUPPORTED
    # empty operands are a no-op
    assert sfwd(0, 8, 64, lens(0, 0), 2, q=null) == 0
    assert sbwd(0, 8, 64, null, 0) == 0
    assert lib.ws_sphere_attention_bwd_scratch_bytes(100, 64) >= 100 * 65 * 4
    assert lib.ws_channel_attention_scratch_bytes(lens(4, 6), 2, 8, 1) > lib.ws_channel_attention_scratch_bytes(lens(4, 6), 2, 8, 0) > 0


def test_attention_operators_refuse_cpu_tensors():
    from weasal_amd import _lib, ops
    x = torch.zeros((4, 8))
    with pytest.raises(_lib.WeasalHipError, match="no CPU fallback"):
        ops.sphere_attention(x, x, torch.zeros((4, 64)), [4])
    with pytest.raises(_lib.WeasalHipError, match="no CPU fallback"):
        ops.channel_attention(x, x, x, [4], True)
