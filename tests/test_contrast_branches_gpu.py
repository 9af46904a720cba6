"""Every instantiation and launch branch of the contrastive-loss kernels (weasal_amd/csrc/contrast_mfma.hip,
contrast_head.hip) against the float64 references of oracle/contrast_branch_ref.py, each C entry on its own with synthetic
inputs, every output element held to the per-element bound derived there (or compared exactly where the reference says so).

The case tables and the data patterns live in the oracle module (tests/test_contrast_branches_cpu.py asserts that they
straddle every threshold and reach every branch).  Outputs are poisoned with NaN before each call, so that an unwritten
element shows; every call runs twice and must repeat its bits.  Each test prints `RATIO <output> <worst |got - ref| / bound>
<elements>` (DESIGN.md section 2 records them).
"""
import numpy as np
import pytest
import torch

from oracle import contrast_branch_ref as R
from weasal_amd import _lib
from weasal_amd._lib import check, current_stream, ptr

pytestmark = pytest.mark.gpu

WS_ERR_INVALID, WS_ERR_UNSUPPORTED = 1, 2
EPS = float(np.float32(1e-8))


def _f32(v):
    return float(np.float32(v))


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _nan(shape, gpu):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=gpu)


def _poison_bytes(nbytes, gpu):
    return torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device=gpu)       # 0xFFFFFFFF: a NaN, or -1


def _held(name, got, ref, bound):
    """every element finite and within its bound; prints the worst ratio"""
    got = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, np.float64)
    ref, bound = np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if got.size == 0:
        return
    assert np.isfinite(got).all(), "%s: %d elements not finite (unwritten?)" % (name, int((~np.isfinite(got)).sum()))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    w = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.ndim else ()
    print("RATIO %s %.4f %d" % (name, float(ratio.max()), got.size))
    assert ratio.max() <= 1.0, "%s: element %s got %r ref %r bound %r" % (name, w, got[w], ref[w], bound[w])


# ------------------------------------------------------------------------------------------------------------------
# rows
# ------------------------------------------------------------------------------------------------------------------
def _rows_fwd(gpu, t, c, n, s, temperature, eps):
    out = [_nan((n,), gpu) for _ in range(4)]
    rc = _lib.lib().ws_contrast_rows_fwd(ptr(t["on"]), n, c, ptr(t["xs"]), s, ptr(t["slc_idx"]), ptr(t["certain"]), ptr(t["lbl"]),
                                         temperature, eps, *[ptr(o) for o in out], current_stream())
    return rc, out


def _rows_bwd(gpu, t, c, n, s, temperature, rowmax, den, npos):
    lib = _lib.lib()
    d_on, d_xs = _nan((n, c), gpu), _nan((s, c), gpu)
    scratch = _poison_bytes(lib.ws_contrast_rows_bwd_scratch_bytes(n, c, s), gpu)
    rc = lib.ws_contrast_rows_bwd(ptr(t["on"]), n, c, ptr(t["xs"]), s, ptr(t["slc_idx"]), ptr(t["certain"]), ptr(t["lbl"]),
                                  temperature, ptr(rowmax), ptr(den), ptr(npos), ptr(t["g"]), ptr(d_on), ptr(d_xs),
                                  ptr(scratch), current_stream())
    return rc, d_on, d_xs


@pytest.mark.parametrize("case", R.ROWS_CASES, ids=[r[0] for r in R.ROWS_CASES])
def test_rows_kernels_hold_the_float64_bounds(gpu, case):
    _id, c, n, s, temperature, pattern = case
    d = R.make_rows_case(c, n, s, pattern)
    t = {k: _dev(v, gpu) for k, v in d.items()}
    T = _f32(temperature)
    ref = R.rows_ref(d["on"], d["xs"], d["slc_idx"], d["certain"], d["lbl"], T, EPS)
    rc, (loss, rowmax, den, npos) = _rows_fwd(gpu, t, c, n, s, T, EPS)
    check(rc)
    _held("loss", loss, ref["loss"], ref["b_loss"])
    _held("rowmax", rowmax, ref["rowmax"], ref["b_rowmax"])
    _held("den", den, ref["den"], ref["b_den"])
    assert np.array_equal(npos.cpu().numpy().astype(np.float64), ref["npos"])
    p0 = ref["npos"] == 0
    assert (loss.cpu().numpy()[p0] == 0).all()                       # no positive column: exactly 0
    rc, again = _rows_fwd(gpu, t, c, n, s, T, EPS)
    check(rc)
    for a, b in zip((loss, rowmax, den, npos), again):
        assert torch.equal(a, b)
    # the backward on its own: the saved statistics are the reference's, rounded to float32
    st = [ref["rowmax"].astype(np.float32), ref["den"].astype(np.float32), ref["npos"].astype(np.float32)]
    bref = R.rows_bwd_ref(d["on"], d["xs"], d["slc_idx"], d["certain"], d["lbl"], T, EPS, d["g"], *st)
    std = [_dev(a, gpu) for a in st]
    rc, d_on, d_xs = _rows_bwd(gpu, t, c, n, s, T, *std)
    check(rc)
    _held("d_on", d_on, bref["d_on"], bref["b_d_on"])
    _held("d_xs", d_xs, bref["d_xs"], bref["b_d_xs"])
    dead = p0 | (d["g"] == 0)
    assert not d_on.cpu().numpy()[dead].any()                         # P = 0 or g = 0: an exactly zero d_on row
    rc, d_on2, d_xs2 = _rows_bwd(gpu, t, c, n, s, T, *std)
    check(rc)
    assert torch.equal(d_on, d_on2) and torch.equal(d_xs, d_xs2)


def test_rows_refusals(gpu):
    """C = 17 and s = 1025 are UNSUPPORTED, a temperature outside [0.023, 1e26] is INVALID (no launch in either case);
    n = 0 is accepted and gives d_xs = 0"""
    lib = _lib.lib()
    for c, n, s, temperature, want in ((17, 20, 40, 0.1, WS_ERR_UNSUPPORTED), (9, 20, 1025, 0.1, WS_ERR_UNSUPPORTED),
                                       (9, 20, 40, 0.02, WS_ERR_INVALID), (9, 20, 40, 0.0, WS_ERR_INVALID),
                                       (9, 20, 40, -0.1, WS_ERR_INVALID), (9, 20, 40, float("nan"), WS_ERR_INVALID),
                                       (9, 20, 40, float("inf"), WS_ERR_INVALID)):
        d = R.make_rows_case(c, n, s, "mixed")
        t = {k: _dev(v, gpu) for k, v in d.items()}
        rc, outs = _rows_fwd(gpu, t, c, n, s, temperature, EPS)
        assert rc == want, (c, s, temperature, rc)
        assert all(bool(torch.isnan(o).all()) for o in outs)
        z = torch.zeros(n, device=gpu)
        rc, d_on, d_xs = _rows_bwd(gpu, t, c, n, s, temperature, z, z + 1, z)
        assert rc == want and bool(torch.isnan(d_on).all()) and bool(torch.isnan(d_xs).all())
    lib.ws_last_error()
    d = R.make_rows_case(9, 8, 40, "mixed")
    t = {k: _dev(v[:0] if k in ("on", "certain", "lbl", "g") else v, gpu) for k, v in d.items()}
    rc, _outs = _rows_fwd(gpu, t, 9, 0, 40, _f32(0.1), EPS)
    check(rc)
    z = torch.zeros(0, device=gpu)
    rc, _d_on, d_xs = _rows_bwd(gpu, t, 9, 0, 40, _f32(0.1), z, z, z)
    check(rc)
    assert not d_xs.cpu().numpy().any() and d_xs.shape == (40, 9)


# ------------------------------------------------------------------------------------------------------------------
# head
# ------------------------------------------------------------------------------------------------------------------
def _head_fwd(gpu, xd, c, labels, threshold, u, r, s):
    lib = _lib.lib()
    n = xd.shape[0]
    o = dict(on=_nan((n, c), gpu), inv_norm=_nan((n,), gpu),
             certain=torch.full((n,), 0xEE, dtype=torch.uint8, device=gpu),
             lbl=torch.full((n,), -77, dtype=torch.int64, device=gpu),
             slc_idx=torch.full((s,), -77, dtype=torch.int64, device=gpu), xs=_nan((s, c), gpu),
             state=torch.full((2,), -77, dtype=torch.int32, device=gpu))
    scratch = _poison_bytes(lib.ws_contrast_head_scratch_bytes(n), gpu)
    rc = lib.ws_contrast_head_fwd(ptr(xd), n, c, xd.stride(0), ptr(labels), threshold, ptr(u), ptr(r), s, ptr(o["on"]),
                                  ptr(o["inv_norm"]), ptr(o["certain"]), ptr(o["lbl"]), ptr(o["slc_idx"]), ptr(o["xs"]),
                                  ptr(o["state"]), ptr(scratch), current_stream())
    return rc, o


HEAD_RUNS = [(r, form) for r in R.HEAD_CASES for form in (("u", "r") if r[2] < 1000000 else ("u",))]


@pytest.mark.parametrize("case,form", HEAD_RUNS, ids=["%s-%s" % (r[0], f) for r, f in HEAD_RUNS])
def test_head_forward_and_selection(gpu, case, form):
    _id, c, n, s, pad, threshold, scale, valid = case
    x, labels = R.make_head_case(c, n, s, pad, scale, valid)
    thr = _f32(threshold)
    h = R.head_ref(x[:, :c], labels, thr)
    rng = R._rng("draw", _id, form)
    if form == "u":
        draw = rng.random(s).astype(np.float32)
        draw = np.minimum(draw, np.nextafter(np.float32(1), np.float32(0)))
        draw[0] = 0.0
        draw[-1] = np.nextafter(np.float32(1), np.float32(0))           # (s = 1: the largest float below 1 alone)
    else:
        nv_ref = max(int(h["certain"].sum()), 1)
        draw = rng.integers(0, nv_ref, size=s).astype(np.int64)
        draw[-1] = nv_ref + 5                                           # beyond the list: clamped to the last valid point
    xd, ld, dd = _dev(x, gpu), _dev(labels, gpu), _dev(draw, gpu)
    u, r = (dd, None) if form == "u" else (None, dd)
    rc, o = _head_fwd(gpu, xd, c, ld, thr, u, r, s)
    check(rc)
    _held("on", o["on"], h["on"], h["b_on"])
    _held("inv_norm", o["inv_norm"], h["inv_norm"], h["b_inv_norm"])
    cert = o["certain"].cpu().numpy()
    lbl = o["lbl"].cpu().numpy()
    assert set(np.unique(cert).tolist()) <= {0, 1}
    ok = ~h["undecided"]
    assert np.array_equal(cert[ok].astype(bool), h["certain"][ok]) and np.array_equal(lbl[ok], h["lbl"][ok])
    given = labels < 10
    assert cert[given].all() and np.array_equal(lbl[given], labels[given])          # a given label, -1 included, is certain
    assert (lbl[~given] >= 0).all() and (lbl[~given] < c).all()                      # so no uncertain point has a negative label
    if n > 7:
        assert not o["on"][7].cpu().numpy().any()                                    # the all-zero row
    # the selection, against the kernel's own certain: exact, no exclusions
    want, nv = R.select_ref(cert, draw, s, n)
    assert np.array_equal(o["slc_idx"].cpu().numpy(), want)
    assert o["state"].cpu().numpy().tolist() == [nv, 0]
    assert torch.equal(o["xs"], o["on"][o["slc_idx"]])
    rc, o2 = _head_fwd(gpu, xd, c, ld, thr, u, r, s)
    check(rc)
    for k in o:
        assert torch.equal(o[k], o2[k]), k


def test_head_refusals(gpu):
    """one slice-length limit for every entry: s = 1025 is refused by the head before any launch, and by ops.contrast_loss"""
    from weasal_amd import ops
    x, labels = R.make_head_case(9, 300, 1025, 0, 1.5, "spread")
    xd, ld = _dev(x, gpu), _dev(labels, gpu)
    u = torch.rand(1025, device=gpu)
    rc, o = _head_fwd(gpu, xd, 9, ld, 0.2, u, None, 1025)
    assert rc == WS_ERR_UNSUPPORTED and bool(torch.isnan(o["on"]).all()) and o["state"].cpu().tolist() == [-77, -77]
    rc = _lib.lib().ws_contrast_head_bwd(ptr(o["on"]), ptr(o["xs"]), ptr(o["slc_idx"]), 1025, ptr(o["on"]), ptr(o["inv_norm"]),
                                         300, 9, ptr(o["on"]), 9, current_stream())
    assert rc == WS_ERR_UNSUPPORTED
    launches = _lib.lib().ws_launch_count() if hasattr(_lib.lib(), "ws_launch_count") else None
    for bad in (dict(draw=u), dict(draw=u[:1000], temperature=0.02), dict(draw=u[:1000], temperature=0.0),
                dict(draw=u[:1000], temperature=-1.0)):
        with pytest.raises(_lib.WeasalHipError):
            ops.contrast_loss(xd, ld, bad["draw"], 0.2, temperature=bad.get("temperature", 0.1))
    if launches is not None:
        assert _lib.lib().ws_launch_count() == launches                 # refused before the first launch
    on = torch.nn.functional.normalize(xd, dim=1)
    idx = torch.zeros(1025, dtype=torch.int64, device=gpu)
    with pytest.raises(_lib.WeasalHipError):
        ops.contrast_rows(on, on[idx], idx, ld < 10, ld.clamp(0, 8), 0.1, 1e-8)


# ------------------------------------------------------------------------------------------------------------------
# tail
# ------------------------------------------------------------------------------------------------------------------
def _tail_fwd(gpu, v, lbl, n, n_cls, state, scratch):
    per_class, w_cls, loss = _nan((n_cls,), gpu), _nan((n_cls,), gpu), _nan((1,), gpu)
    check(_lib.lib().ws_contrast_tail_fwd(ptr(v), ptr(lbl), n, n_cls, ptr(state), ptr(per_class), ptr(w_cls), ptr(loss),
                                          ptr(scratch), current_stream()))
    return per_class, w_cls, loss


@pytest.mark.parametrize("n,n_cls", R.TAIL_CASES)
def test_tail_forward_and_backward(gpu, n, n_cls):
    lib = _lib.lib()
    v, lbl = R.make_tail_case(n, n_cls)
    vd, ld = _dev(v, gpu), _dev(lbl, gpu)
    ref = R.tail_ref(v, lbl, n_cls, 5)
    state = torch.tensor([5, 0], dtype=torch.int32, device=gpu)
    scratch = _poison_bytes(lib.ws_contrast_tail_scratch_bytes(n), gpu)
    per_class, w_cls, loss = _tail_fwd(gpu, vd, ld, n, n_cls, state, scratch)
    assert state.cpu().tolist() == [5, 0]                               # the arrival counter is back at 0
    pc = per_class.cpu().numpy()
    if ref["sel"].any():
        _held("per_class", per_class, ref["per_class"], ref["b_per_class"])
        _held("w_cls", w_cls, ref["w_cls"], ref["b_w_cls"])
        _held("tail_loss", loss, [ref["loss"]], [ref["b_loss"]])
        assert np.array_equal(pc > 0, ref["sel"]) and (pc[~ref["sel"]] == 0).all()
    else:                                                               # no class kept: 0 / 0 like the reference's empty mean
        assert np.isnan(ref["loss"]) and bool(torch.isnan(loss).all()) and not pc.any()
    again = _tail_fwd(gpu, vd, ld, n, n_cls, state, scratch)
    assert state.cpu().tolist() == [5, 0]
    for a, b in zip((per_class, w_cls, loss), again):
        assert torch.equal(a, b, ) or (bool(torch.isnan(a).all()) and bool(torch.isnan(b).all()))
    # the gradient coefficient: one float32 product per kept point, exact
    g = torch.tensor([1.7], device=gpu)
    g_row = _nan((n,), gpu)
    check(lib.ws_contrast_tail_bwd(ptr(vd), ptr(ld), n, n_cls, ptr(w_cls), ptr(g), ptr(g_row), current_stream()))
    want = R.tail_bwd_ref(v, lbl, n_cls, w_cls.cpu().numpy(), np.float32(1.7))
    assert np.array_equal(g_row.cpu().numpy(), want, equal_nan=True)
    # no valid point: loss 0 and no gradient, whatever the losses are
    none = torch.zeros(2, dtype=torch.int32, device=gpu)
    _pc0, w0, l0 = _tail_fwd(gpu, vd, ld, n, n_cls, none, scratch)
    assert float(l0) == 0.0 and not w0.cpu().numpy().any() and none.cpu().tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------------------------
# head backward
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.HEAD_BWD_CASES, ids=["c%d_n%d_s%d_%s" % (r[0], r[1], r[2], r[4]) for r in R.HEAD_BWD_CASES])
def test_head_backward(gpu, case):
    c, n, s, pad, pattern = case
    d = R.make_head_bwd_case(c, n, s, pattern)
    t = {k: _dev(v, gpu) for k, v in d.items()}

    def run():
        d_on = t["d_on"].clone()
        d_x = _nan((n, c + pad), gpu)
        check(_lib.lib().ws_contrast_head_bwd(ptr(d_on), ptr(t["d_xs"]), ptr(t["slc_idx"]), s, ptr(t["on"]), ptr(t["inv_norm"]),
                                              n, c, ptr(d_x), c + pad, current_stream()))
        return d_on, d_x

    d_on, d_x = run()
    want = R.slice_add_ref(d["d_on"], d["d_xs"], d["slc_idx"])
    assert np.array_equal(d_on.cpu().numpy(), want)                      # float32, slot order: bitwise
    ref, bound = R.normalize_bwd_ref(want, d["on"], d["inv_norm"])
    _held("d_x", d_x[:, :c], ref, bound)
    assert bool(torch.isnan(d_x[:, c:]).all())                           # the columns beyond c stay untouched (ldd > c)
    d_on2, d_x2 = run()
    assert torch.equal(d_on, d_on2) and torch.equal(d_x[:, :c], d_x2[:, :c])
