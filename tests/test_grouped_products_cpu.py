"""CPU: the block scratch-size queries with the grouped product launches on and off (host planning code only: ws_kpblock_* /
ws_upunary_*_scratch_bytes, weasal_amd/csrc/blocks.hip).  Grouping gives every member of a group its own partial-sum
scratch -- a sum where the single launches share the maximum -- so over a grid of block shapes the grouped query must be
finite, 256-aligned and at least the ungrouped one; above the row limit, and with the switch at 0, it is the ungrouped one."""
import ctypes as C
import itertools

import pytest

from weasal_amd import _lib, fused

FAKE = 0x10000          # a 16-byte aligned address: the size queries read no memory


def _switch(lib):
    return C.c_int64.in_dll(lib, "ws_block_group_rows")


def _kp(nq, ns, in_dim, conv, out_dim, strided, w1, w2, ws, dfeat):
    d = fused.KPBlockDesc()
    for f in ("q_pts", "s_pts", "inds", "kernel_points", "feat", "wk", "wf", "out", "dout", "dwk"):
        setattr(d, f, FAKE)
    d.nq, d.ns, d.h, d.k, d.extent, d.slope = nq, ns, 20, 15, 1.0, 0.1
    d.in_dim, d.conv_in, d.conv_out, d.out_dim, d.strided = in_dim, conv, conv, out_dim, strided
    if w1:
        d.w1 = d.x1 = d.dw1 = FAKE
    if w2:
        d.w2 = d.x2 = d.dw2 = FAKE
        if strided:
            d.pooled = d.arg = FAKE
    if ws:
        d.ws = d.dws = FAKE
    if dfeat:
        d.dfeat = FAKE
    return d


def _shapes():
    for (nq, strided), (in_dim, out_dim), dfeat in itertools.product(
            [(0, 0), (1, 0), (33, 0), (700, 0), (700, 1), (4000, 0), (32767, 0), (32768, 0), (71000, 0), (71000, 1)],
            [(64, 128), (128, 128), (128, 512), (512, 1024)], [0, 1]):
        ns = nq if not strided else nq * 3
        mid = out_dim // 4
        yield _kp(nq, ns, in_dim, mid, out_dim, strided, in_dim != mid, True, in_dim != out_dim, dfeat)       # resnet block
    for nq in (0, 50, 700, 40000):
        yield _kp(nq, nq, 64, 64, 64, 0, False, False, False, 1)                                               # simple block


def test_block_scratch_queries_with_grouping_on_and_off():
    lib = fused._bind()
    sw = _switch(lib)
    default = sw.value
    assert default > 0
    grew = 0
    try:
        for d in _shapes():
            sizes = {}
            for value in (0, default, 1 << 62):
                sw.value = value
                for name in ("ws_kpblock_fwd_scratch_bytes", "ws_kpblock_bwd_scratch_bytes"):
                    n = getattr(lib, name)(C.byref(d))
                    assert 256 <= n < (1 << 40) and n % 256 == 0, (name, value, d.nq, n, lib.ws_last_error())
                    sizes[name, value] = n
            for name in ("ws_kpblock_fwd_scratch_bytes", "ws_kpblock_bwd_scratch_bytes"):
                assert sizes[name, 0] <= sizes[name, default] <= sizes[name, 1 << 62], (name, d.nq, sizes)
                if max(d.nq, d.ns) >= default or d.nq == 0:
                    assert sizes[name, default] == sizes[name, 0], (name, d.nq, sizes)         # above the limit / empty: the single launches
                grew += sizes[name, default] > sizes[name, 0]
    finally:
        sw.value = default
    assert grew >= 8            # the short resnet blocks do take a scratch per member


@pytest.mark.parametrize("nc,nf", [(0, 0), (37, 300), (4000, 20000), (20000, 71000)])
def test_decoder_step_scratch_queries(nc, nf):
    lib = fused._bind()
    sw = _switch(lib)
    default = sw.value
    u = fused.UpUnaryDesc()
    for f in ("xc", "skip", "ups", "w", "out"):
        setattr(u, f, FAKE)
    u.nc, u.nf, u.c_up, u.c_skip, u.out_dim, u.ldw, u.h_up = nc, nf, 256, 128, 128, 384, 1
    try:
        got = {}
        for value in (0, default):
            sw.value = value
            got[value] = [getattr(lib, n)(C.byref(u)) for n in ("ws_upunary_fwd_scratch_bytes", "ws_upunary_bwd_scratch_bytes")]
            assert all(256 <= n < (1 << 40) and n % 256 == 0 for n in got[value]), got
    finally:
        sw.value = default
    assert got[default][0] == got[0][0] and got[default][1] >= got[0][1]
    if 0 < max(nc, nf) < default:
        assert got[default][1] > got[0][1]
    else:
        assert got[default][1] == got[0][1]
