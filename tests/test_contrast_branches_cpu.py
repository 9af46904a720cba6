"""The references of oracle/contrast_branch_ref.py and the case tables of tests/test_contrast_branches_gpu.py, checked on
the CPU: the references compose to oracle/contrast_ref.py; each bound rejects each deliberately wrong reference; the tables
straddle every threshold of the launchers and reach every instantiation / launch branch; the inputs hold what the cases
rely on."""
import numpy as np
import pytest
import torch

from oracle import contrast_branch_ref as R
from oracle.contrast_ref import contrast_loss_ref

SMALL = [r for r in R.ROWS_CASES if r[2] <= 300]           # the teeth run on the cases a CPU does in a moment


def _ref_case(seed, n, c, n_labeled, sharp):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, c, generator=g) * sharp).double()
    labels = torch.full((n,), 100, dtype=torch.int64)
    idx = torch.randperm(n, generator=g)[:n_labeled]
    labels[idx] = torch.randint(0, min(c, 9), (n_labeled,), generator=g)
    return x, labels


@pytest.mark.parametrize("seed,n,c,n_labeled,sharp,thd", [(0, 1400, 9, 100, 2.0, 10),      # num_valid >= 1000
                                                          (1, 400, 9, 30, 0.05, 60),       # the padded slice
                                                          (2, 300, 4, 0, 0.01, 99),        # nothing valid
                                                          (3, 350, 16, 350, 1.0, 10),      # fully labelled, the widest rows
                                                          (4, 200, 1, 20, 1.0, 10)])
def test_references_compose_to_the_loss(seed, n, c, n_labeled, sharp, thd):
    x, labels = _ref_case(seed, n, c, n_labeled, sharp)
    h = R.head_ref(x.numpy(), labels.numpy(), thd / 100)
    nv = int(h["certain"].sum())
    g = torch.Generator().manual_seed(seed + 1)
    draw = torch.zeros(0, dtype=torch.int64) if nv == 0 else \
        torch.randint(0, nv, (1000 if nv >= 1000 else 1000 - nv,), generator=g)
    xr = x.clone().requires_grad_(True)
    ref = contrast_loss_ref(xr, labels, thd, draw)
    r = draw.numpy() if nv >= 1000 else np.concatenate([np.arange(nv), draw.numpy()])
    if nv == 0:
        r = np.zeros(1000, np.int64)
    got = R.composed_loss_ref(x.numpy(), labels.numpy(), thd / 100, r, n_cls=max(c, 10))
    assert got["num_valid"] == nv
    if nv == 0:
        assert float(ref) == 0.0 and got["loss"] == 0.0 and not got["d_x"].any()
        assert (got["slc_idx"] == n - 1).all()
        return
    assert abs(got["loss"] - float(ref.detach())) <= 1e-10 * abs(float(ref.detach()))
    ref.backward()
    gr = xr.grad.numpy()
    # (C = 1: the normalised rows are +-1 and the true gradient is 0; both sides hold cancellation residue of 1e-15)
    assert np.abs(got["d_x"] - gr).max() <= 1e-9 * np.abs(gr).max() + 1e-13


def test_select_ref_rules():
    cert = np.zeros(50, bool)
    cert[[3, 10, 11, 40]] = True
    u = np.array([0.0, np.nextafter(np.float32(1), np.float32(0)), 0.5, 0.99, 0.3, 0.1], np.float32)
    slc, nv = R.select_ref(cert, u, 6)
    assert nv == 4 and slc.tolist() == [3, 10, 11, 40, 10, 3]          # fewer valid points than slots: each once first
    slc, _ = R.select_ref(cert, u[:3], 3)                               # nv >= s: the draws alone
    assert slc.tolist() == [3, 40, 11]
    slc, _ = R.select_ref(cert, np.array([2, 7, -1], np.int64), 3)      # given positions, clamped
    assert slc.tolist() == [11, 40, 3]
    slc, nv = R.select_ref(np.zeros(9, bool), u, 6)
    assert nv == 0 and slc.tolist() == [8] * 6
    # the largest float below 1 times a large count rounds up to the count itself: the clamp holds it
    big = np.ones(1 << 20, bool)
    assert R.select_ref(big, u[1:2], 1)[0][0] == (1 << 20) - 1


def test_slice_add_ref_is_slot_ordered_float32():
    d_on = np.array([[1.0], [1e8]], np.float32)
    d_xs = np.array([[1.0], [-1e8], [3.0]], np.float32)
    out = R.slice_add_ref(d_on, d_xs, np.array([1, 1, 1]))
    assert out.dtype == np.float32 and out[1, 0] == np.float32(np.float32(np.float32(1e8) + 1) - np.float32(1e8)) + 3
    assert out[0, 0] == 1.0


def _exceeds(ref, mut):
    bad = not np.array_equal(ref["npos"], mut["npos"])
    for k in ("loss", "rowmax", "den"):
        bad = bad or bool((np.abs(mut[k] - ref[k]) > ref["b_" + k]).any())
    return bad


def _applies(mutation, c, n, s, d):
    if mutation == "pad":
        return s % 16 != 0
    if mutation == "xs_hi":
        return c > 12
    if mutation == "dup_last":
        return n % 16 != 0 and n >= 2
    if mutation == "self":
        return np.unique(d["slc_idx"]).size < s and n > 1
    return True


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_the_bound_rejects_a_wrong_reference(mutation):
    """a reference wrong in one way exceeds the bound of the right one: on some case of the table, and for the
    layout-dependent mutations on a case of every instantiation NS = ceil(C / 4) they can occur in"""
    caught = {}
    for _id, c, n, s, t, pattern in SMALL:
        d = R.make_rows_case(c, n, s, pattern)
        if not _applies(mutation, c, n, s, d):
            continue
        args = (d["on"], d["xs"], d["slc_idx"], d["certain"], d["lbl"], t, 1e-8)
        ns = (c + 3) // 4
        caught[ns] = caught.get(ns, False) or _exceeds(R.rows_ref(*args), R.rows_ref(*args, mutate=mutation))
    assert any(caught.values()), mutation
    if mutation in R.LAYOUT_MUTATIONS:
        want = {4} if mutation == "xs_hi" else {1, 2, 3, 4}
        assert {k for k, v in caught.items() if v} >= want, (mutation, caught)


def test_a_float32_restatement_stays_inside_the_bounds():
    """the bounds are not too tight either: the same formulas in float32 numpy (two-pass) stay inside them"""
    f = np.float32
    for _id, c, n, s, t, pattern in SMALL[::3]:
        d = R.make_rows_case(c, n, s, pattern)
        ref = R.rows_ref(d["on"], d["xs"], d["slc_idx"], d["certain"], d["lbl"], t, 1e-8)
        use, pos = R._masks(n, d["slc_idx"], d["certain"], d["lbl"])
        mul = (d["on"] @ d["xs"].T) * (f(1) / f(t))
        m = mul.max(1)
        ex = np.where(use, np.exp(mul - m[:, None]), f(0)).astype(f)
        den = ex.sum(1, dtype=f) + f(1e-8)
        P = pos.sum(1).astype(f)
        S = np.where(pos, mul, f(0)).sum(1, dtype=f)
        loss = -f(t) * (((S - P * m) - P * np.log(den)) / (P + f(1e-12)))
        for k, got in (("loss", loss), ("rowmax", m), ("den", den)):
            assert (np.abs(got - ref[k]) <= ref["b_" + k]).all(), (_id, k)
        b = R.rows_bwd_ref(d["on"], d["xs"], d["slc_idx"], d["certain"], d["lbl"], t, 1e-8, d["g"], m, den, P)
        gc = d["g"] * (-f(t) / (P + f(1e-12))) / f(t)
        W = gc[:, None] * (pos.astype(f) - np.where(use, P[:, None] * np.exp(mul - m[:, None]) / den[:, None], f(0)))
        W = W.astype(f)
        assert (np.abs(W @ d["xs"] - b["d_on"]) <= b["b_d_on"]).all(), _id
        assert (np.abs(W.T @ d["on"] - b["d_xs"]) <= b["b_d_xs"]).all(), _id


def test_tables_straddle_every_threshold():
    mixed = [r for r in R.ROWS_CASES if r[5] == "mixed"]
    cs = {r[1] for r in mixed if r[2:4] == (257, 1000)}
    assert cs >= {1, 4, 5, 8, 9, 12, 13, 16}
    ss = {r[3] for r in R.ROWS_CASES if r[1] == 9}
    assert ss >= {1, 15, 16, 17, 1000, 1024}
    ns = {r[2] for r in R.ROWS_CASES if r[1] == 9 and r[3] == 1000}
    assert ns >= {1, 16, 17, 255, 256, 257, 8192, 8193}
    assert {r[4] for r in R.ROWS_CASES} >= {0.05, 0.1, 1.0}
    assert (1, 1, 1) in {r[1:4] for r in R.ROWS_CASES} and (16, 8193, 1024) in {r[1:4] for r in R.ROWS_CASES}
    assert {r[5] for r in R.ROWS_CASES} == set(R.ROWS_PATTERNS)
    tn = {n for n, _k in R.TAIL_CASES}
    assert tn >= {1, 4095, 4096, 4097, 524288, 524289} and {k for _n, k in R.TAIL_CASES} >= {1, 10, 16}
    hn = {r[2] for r in R.HEAD_CASES}
    assert hn >= {1, 255, 256, 257, 70001, 2097152, 2097153}
    assert {r[3] for r in R.HEAD_CASES} >= {1, 63, 64, 65, 1000, R.S_MAX}
    assert {r[1] for r in R.HEAD_CASES} >= {1, 2, 9, 10, 15, 16} and any(r[4] > 0 for r in R.HEAD_CASES)
    assert {r[2] for r in R.HEAD_BWD_CASES if True} and {r[2] for r in R.HEAD_BWD_CASES} >= {1, 4, 5, 64, 65, 1000}
    assert {r[0] for r in R.HEAD_BWD_CASES} >= {1, 9, 16} and any(r[3] > 0 for r in R.HEAD_BWD_CASES)


def test_tables_reach_every_instantiation_and_launch_branch():
    rows = set()
    for _id, c, n, s, _t, _p in R.ROWS_CASES:
        rows |= R.rows_plan(c, n, s)
    assert rows >= {"NS1", "NS2", "NS3", "NS4", "c%4=0", "c%4=1", "tile_partial", "tile_full", "s_lt16", "s_padded", "s_tiles",
                    "partial_is_d_xs", "partial_is_d_xs_c=9", "partial_is_d_xs_c!9", "scratch", "reduce_1trip", "reduce_2trips"}
    head = set()
    for r in R.HEAD_CASES:
        head |= R.head_plan(r[2], r[3])
    assert head >= {"rpb256", "rpb512", "blocks1", "blocks_many", "select_grid1", "select_grid2", "select_grid3"}
    assert R.head_plan(2097152, 1000) >= {"rpb256"} and R.head_plan(2097153, 1000) >= {"rpb512"}
    tail = set()
    for n, _k in R.TAIL_CASES:
        tail |= R.tail_plan(n)
    assert tail >= {"tail_blocks1", "tail_blocks_many", "stage_passes1", "stage_passes2"}
    assert "stage_passes1" in R.tail_plan(524288) and "stage_passes2" in R.tail_plan(524289)


def test_rows_inputs_hold_what_the_cases_rely_on():
    seen = set()
    for _id, c, n, s, t, pattern in SMALL:
        d = R.make_rows_case(c, n, s, pattern)
        assert np.array_equal(d["xs"], d["on"][d["slc_idx"]])
        nrm = np.sqrt((d["on"].astype(np.float64) ** 2).sum(1))
        assert ((np.abs(nrm - 1) < 1e-6) | (nrm == 0)).all()              # the unit-row precondition (or an all-zero row)
        assert (d["lbl"] >= 0).all()
        use, pos = R._masks(n, d["slc_idx"], d["certain"], d["lbl"])
        if n >= 8 and pattern in ("mixed", "valid_slice", "repeat", "one_point"):
            assert not d["on"][0].any() and d["on"][1, 0] == 1.0 and d["on"][2, c - 1] == -1.0
            assert d["lbl"][3] == 9 and pos[4].sum() == 0 and 4 not in d["slc_idx"]
            seen.add("P0")
        if pattern == "valid_slice":
            unc = d["certain"] == 0
            assert unc.any() and use[unc].sum() == 0 and d["certain"][d["slc_idx"]].all()
            seen.add("E0")
        if pattern == "repeat":
            slots = np.nonzero(d["slc_idx"] == 6)[0]
            assert {0, 15, 16, 17, 31, 32} <= set(slots.tolist()) and s - 1 in slots
            seen.add("repeat")
        if pattern == "one_point":
            assert np.unique(d["slc_idx"]).size == 1
            seen.add("one_point")
        if pattern == "one_label":
            assert d["certain"].all() and np.unique(d["lbl"]).size == 1
            seen.add("one_label")
        if c == 16 and pattern == "mixed":
            assert d["lbl"][np.arange(n) != 4].max() == 15 or n < 64
        g = d["g"]
        if n >= 100:
            assert (g == 0).any() and (g > 0).any() and (g < 0).any()
            nz = np.abs(g[g != 0])
            assert nz.max() / nz.min() > 1e4
    assert seen == {"P0", "E0", "repeat", "one_point", "one_label"}


@pytest.mark.parametrize("case", [r for r in R.HEAD_CASES], ids=[r[0] for r in R.HEAD_CASES])
def test_head_inputs_and_the_exclusion_cap(case):
    """at most 1 % of a case's rows may be left out of the certain / lbl comparison (the float64 max-probability within
    1e-5 of the threshold, or the top two probabilities within 1e-5 relative); the valid points lie where the case says"""
    _id, c, n, s, pad, thr, scale, valid = case
    x, labels = R.make_head_case(c, n, s, pad, scale, valid)
    h = R.head_ref(x[:, :c], labels, thr)
    assert h["undecided"].sum() <= 0.01 * n, (h["undecided"].sum(), n)
    cert = h["certain"]
    idx = np.nonzero(cert)[0]
    if valid == "none":
        assert idx.size == 0
    elif valid == "one":
        assert idx.size == 1
    elif valid == "first":
        assert idx.size and idx.max() < 256
    elif valid == "last":
        assert idx.size and idx.min() >= n - 256
    elif valid == "runs":
        assert idx.size and np.diff(idx).max() > 10000
    elif isinstance(valid, int):
        assert idx.size == valid
    if valid not in ("none",) and n > 1000:
        assert set(labels[labels < 10].tolist()) >= {0, 9, -1} and {10, 100} <= set(labels.tolist())
    if n > 7:
        assert h["inv_norm"][7] == 1e12 and not h["on"][7].any()


def test_tail_and_head_backward_inputs():
    for n, k in R.TAIL_CASES:
        v, lbl = R.make_tail_case(n, k)
        if n >= 4095:
            assert lbl.min() < 0 and lbl.max() >= k and (v == 0).any() and (v < 0).any()
            t = R.tail_ref(v, lbl, k, 1)
            if k >= 10:
                assert t["per_class"][4] == 0 and t["per_class"][6] == 0 and not t["sel"][4] and not t["sel"][6]
            assert t["sel"].any()
    for c, n, s, _pad, pattern in R.HEAD_BWD_CASES:
        d = R.make_head_bwd_case(c, n, s, pattern)
        assert d["inv_norm"][0] >= np.float32(1e12) * (1 - 1e-6) and not d["on"][0].any()
        if pattern == "same":
            assert np.unique(d["slc_idx"]).size == 1
        if pattern == "dups" and s > 65:
            assert {1, 2, 63, 64, 65, s - 1} <= set(np.nonzero(d["slc_idx"] == 3)[0].tolist())


def test_temperature_range_is_derived():
    """the one-pass form needs exp(-2 / T) (1 + a few u) to be a normal float: 2 / T_MIN < 87 < -log(FLT_MIN) = 87.34, and
    the backward's -T / 1e-12 to be finite"""
    assert 2.0 / R.T_MIN < 87.0 < -np.log(float(np.finfo(np.float32).tiny))
    assert np.isfinite(np.float32(R.T_MAX) / np.float32(1e-12))
    assert np.exp(np.float32(-2.0 / R.T_MIN)) >= np.finfo(np.float32).tiny
