"""The packed table walk of K4 (ws_kpconv_gather_bwd_x_packed: kpconv_gather_bwd_x_packed_kernel, four supports per wave)
held to the entry it stands in for, ws_kpconv_gather_bwd_x_gated, bit for bit: torch.equal on the same arguments, no
tolerance.  One case is also held to the float64 reference within its per-element bound, so that the two kernels cannot be
wrong together.

Inputs as in tests/test_kpconv_branches_gpu.py: points on the 2^-6 lattice, kernel points 2^-7 off it
(oracle/kpconv_branch_ref.py), the table from ops.TransposedTable.  The in-degree cases write the index rows by hand: a
support's in-degree decides whether it rides in a 16-lane group (<= 16 pairs), takes the whole wave (more), or overflows
its quarter of the pool (every kernel point live on 16 pairs: 240 entries against 64).  A quad is four consecutive supports
of a workgroup's range (four consecutive entries of the order when one is given); ns = 512 and 32 make the ranges multiples
of 16, so supports 4 t .. 4 t + 3 share a wave.  Every table keeps nq * h <= 8 ns, inside the scope of the packed form.
dx starts as NaN in both runs: a row nobody wrote fails the comparison."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import kpconv_branch_ref as R

pytestmark = pytest.mark.gpu

K = 15
EXTENT = 0.3
RADIUS = 0.75
KP_REACH = 0.7 * EXTENT * 1.5
PACKED = "kpconv_gather_bwd_x_packed_kernel"


def _variant(nq, ns, h, ci, dwf=0x10000000, dx=0x20000000, bf16=False, ordered=False):
    from weasal_amd import _lib, ops
    buf = C.create_string_buffer(256)
    _lib.check(_lib.lib().ws_kpconv_gather_bwd_x_packed_variant(nq, ns, h, ci, dwf, dx, 0, 0, ops.INFLUENCE["linear"], ops.AGGREGATION["sum"],
                                                              int(bf16), int(ordered), buf, 256))
    return buf.value.decode()


def _g(ci):
    return 1 if ci <= 4 else 2 if ci <= 8 else 4 if ci <= 16 else 8 if ci <= 32 else 16


def _degree_rows(deg, nq, live_rows, rng):
    """[nq, h] index rows in which support s appears deg[s] times, never twice in a row; rows >= live_rows are all shadow and
    the unused columns hold the shadow index"""
    ns = len(deg)
    assert max(deg) <= live_rows <= nq
    flat = np.repeat(np.arange(ns), deg)
    h = -(-len(flat) // live_rows) + 1                 # one column more than needed: shadow entries inside live rows
    inds = np.full((nq, h), ns, np.int64)
    slots = rng.permutation(h)                          # the columns in a random order, so that shadows sit between real entries
    for i, s in enumerate(flat):
        inds[i % live_rows, slots[i // live_rows]] = s
    assert np.array_equal(np.bincount(inds[inds < ns], minlength=ns), np.asarray(deg))
    assert all(len(set(r[r < ns])) == (r < ns).sum() for r in inds)
    return inds


DEGREES = [0, 1, 15, 16, 17, 64, 65, 400,        # quads 0 and 1: every boundary of the group / chunk sizes, one hub
           3, 2, 20, 5,                          # quad 2: exactly one support above 16 between three small ones
           0, 0, 0, 0]                           # quad 3: four empty supports


def _degree_case(rng, extent=EXTENT, deg=DEGREES, ns=512, nq=440):
    deg = list(deg) + list(rng.integers(0, 5, size=ns - len(deg)))       # the rest: 0 .. 4 incoming pairs
    s = R.lattice_cloud(rng, ns, 0.4)
    q = R.lattice_cloud(rng, nq, 0.4)
    live = nq - nq // 20                                # the last rows are all shadow
    inds = _degree_rows(deg, nq, live, rng)
    assert (inds[live:] == ns).all() and (inds[:live] == ns).any() and nq * inds.shape[1] <= 8 * ns
    return q, s, inds, extent


def _lattice_case(rng, ns, nq, h):
    s = R.lattice_cloud(rng, ns, 0.8)
    q = R.lattice_cloud(rng, nq, 0.6)
    return q, s, R.brute_rows(q, s, RADIUS, h), EXTENT


_KP = {}


def _kernel():
    if "kp" not in _KP:
        _KP["kp"] = R.lattice_kernel(np.random.default_rng(5), K, KP_REACH)
    return _KP["kp"]


def _both(gpu, q, s, inds, extent, ci, order=False, gate=False, seed=1, entries=("ws_kpconv_gather_bwd_x_packed", "ws_kpconv_gather_bwd_x_gated")):
    """dx of the two entries on the same arguments (and those arguments, for a reference)"""
    from weasal_amd import _lib, ops
    from weasal_amd._lib import check, current_stream, ptr
    lib = _lib.lib()
    nq, ns, h = q.shape[0], s.shape[0], inds.shape[1]
    gen = torch.Generator(device="cpu").manual_seed(seed)
    Q, S, I = torch.from_numpy(q).to(gpu), torch.from_numpy(s).to(gpu), torch.from_numpy(inds).to(gpu)
    table = ops.TransposedTable(I, ns)
    dwf = torch.randn(nq, K, ci, generator=gen).to(gpu)
    kp = torch.from_numpy(_kernel()).to(gpu)
    perm = torch.randperm(ns, generator=gen).to(torch.int32).to(gpu) if order else None
    gy = None
    if gate:                                            # positive, negative and zero values
        gy = torch.randn(ns, ci, generator=gen)
        gy[torch.rand(ns, ci, generator=gen) < 0.2] = 0.0
        assert (gy > 0).any() and (gy < 0).any() and (gy == 0).any()
        gy = gy.to(gpu)
    out = []
    for entry in entries:
        dx = torch.full((ns, ci), float("nan"), device=gpu)
        check(getattr(lib, entry)(ptr(Q), nq, ptr(S), ns, ptr(I), h, ptr(table.offsets), ptr(table.pairs), ptr(dwf), ci, ptr(kp), K, None,
                                  None, extent, ops.INFLUENCE["linear"], ops.AGGREGATION["sum"], ptr(perm), ptr(gy), 0.1, ptr(dx),
                                  current_stream()))
        out.append(dx)
    torch.cuda.synchronize()
    text = _variant(nq, ns, h, ci, dwf.data_ptr(), out[0].data_ptr(), ordered=order)
    return out, text, dwf


def _expect_packed(text, ci):
    assert text.startswith("%s<K=15, G=%d, VEC=true, T=float>" % (PACKED, _g(ci))), text


@pytest.mark.parametrize("ns", [1, 2, 3, 4, 5, 403])
def test_tail_quads(gpu, ns):
    """the last quad of the range holds ns % 4 supports; ns = 1 has no nq < ns with a query in it: the old launch, trivially equal"""
    rng = np.random.default_rng(ns)
    nq = 100 if ns == 403 else max(ns - 1, 1)
    q, s, inds, extent = _lattice_case(rng, ns, nq, 20 if ns == 403 else min(ns, 3))
    assert nq * inds.shape[1] <= 8 * ns
    (packed, gated), text, _ = _both(gpu, q, s, inds, extent, 32)
    if nq < ns:
        _expect_packed(text, 32)
    else:
        assert text == "none"
    assert torch.equal(packed, gated) and not torch.isnan(gated).any()


@pytest.mark.parametrize("ci", [4, 8, 16, 32, 64, 128, 256, 30])
def test_in_degrees_and_row_widths(gpu, ci):
    """supports with 0, 1, 15, 16, 17, 64, 65 and 400 incoming pairs, one large support between three small ones, a quad of
    empty supports, shadow entries and all-shadow rows; every G, several channel chunks (ci = 128, 256: the list is built once),
    and ci = 30, which the packed form does not take"""
    q, s, inds, extent = _degree_case(np.random.default_rng(11))
    (packed, gated), text, _ = _both(gpu, q, s, inds, extent, ci)
    if ci % 4:
        assert text == "none"
    else:
        _expect_packed(text, ci)
    assert torch.equal(packed, gated) and not torch.isnan(gated).any()
    deg = np.bincount(inds[inds < 512], minlength=512)
    assert (gated[torch.from_numpy(deg == 0).to(gpu)] == 0).all() and float(gated[7].abs().max()) > 0


def test_pool_overflow_takes_the_single_support_path(gpu):
    """an extent that keeps all 15 kernel points live on every pair: 16 pairs are 240 entries against the 64 of a group's
    quarter (960 against the 256-entry pool for the quad).  Quads of four such supports, and quads where they sit next to
    small supports whose entries fit"""
    deg = [16, 16, 16, 16, 16, 1, 2, 16, 4, 4, 4, 4, 5, 0, 3, 16]
    q, s, inds, extent = _degree_case(np.random.default_rng(12), extent=10.0, deg=deg, ns=32, nq=24)
    kp = _kernel().astype(np.float64)
    d = np.linalg.norm((s[:, None, None, :].astype(np.float64) - q[None, :, None, :]) - kp[None, None], axis=-1)
    assert d.max() < 10.0                                # every (pair, kernel point) has influence
    for ci in (32, 128):
        (packed, gated), text, _ = _both(gpu, q, s, inds, extent, ci, gate=True)
        _expect_packed(text, ci)
        assert torch.equal(packed, gated) and not torch.isnan(gated).any()


@pytest.mark.parametrize("order", [False, True], ids=["index", "order"])
@pytest.mark.parametrize("gate", [False, True], ids=["plain", "gate"])
@pytest.mark.parametrize("ci", [32, 128])
def test_order_and_gate(gpu, ci, gate, order):
    q, s, inds, extent = _degree_case(np.random.default_rng(13))
    (packed, gated), text, _ = _both(gpu, q, s, inds, extent, ci, order=order, gate=gate)
    _expect_packed(text, ci)
    assert torch.equal(packed, gated) and not torch.isnan(gated).any()


def test_two_runs_are_equal(gpu):
    q, s, inds, extent = _degree_case(np.random.default_rng(14))
    (a, b), _, _ = _both(gpu, q, s, inds, extent, 64, order=True, gate=True, entries=("ws_kpconv_gather_bwd_x_packed",) * 2)
    assert torch.equal(a, b) and not torch.isnan(a).any()


def test_packed_vs_float64(gpu):
    """the packed kernel against the float64 reference within the per-element bound of oracle/kpconv_branch_ref.py"""
    rng = np.random.default_rng(15)
    q, s, inds, extent = _lattice_case(rng, 403, 100, 20)
    kp = _kernel()
    assert R.extent_margin(q, s, inds, kp, EXTENT) > 1e-6
    ci = 32
    (packed, gated), text, dwf = _both(gpu, q, s, inds, extent, ci)
    _expect_packed(text, ci)
    dwf = dwf.cpu().numpy()
    x = np.zeros((s.shape[0], ci), np.float32)
    rdx, _, _ = R.ref_backward(x, dwf, q, s, inds, kp, EXTENT, "linear", "sum")
    tol = R.dx_bound(dwf, q, s, inds, kp, EXTENT, "linear", "sum", None, None, 0.0, rdx, False, x.shape)
    msg = R.describe(packed.cpu().numpy(), rdx, tol, "dx")
    assert not msg, msg
    assert np.abs(np.asarray(rdx)).max() > 0
    assert torch.equal(packed, gated)


def test_reporter_at_the_strided_shapes(gpu):
    """the strided blocks of the DALES step (level 0 to 1, level 1 to 2) take the packed kernel; a self-query layer does not"""
    assert _variant(71000, 400000, 59, 32).startswith(PACKED + "<K=15, G=8, VEC=true, T=float>")
    assert _variant(10257, 71070, 60, 64).startswith(PACKED + "<K=15, G=16, VEC=true, T=float>")
    assert _variant(400000, 400000, 59, 32) == "none"
