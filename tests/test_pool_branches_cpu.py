"""CPU side of tests/test_pool_branches_gpu.py: the references of oracle/pool_ref.py are right, the bound has teeth, and the
case tables cover the launchers' plans.

* max_pool_ref / closest_pool_ref and their float64 backwards agree with the torch restatement (oracle.kpconv_ref, autograd
  on the CPU) on tie-heavy integer data, exactly, and with the g6 golden.
* transposed_table_ref agrees with a brute-force nonzero per support.
* Which form a call takes is asked of the library: ws_pool_variant formats the plan functions the launchers of pools.hip
  dispatch on (no device needed).  The names it gives for the GPU case tables are every name it gives over a sweep of
  widths, row counts, alignments, orders and records; the set is the expected one, counted here from literals; the tables
  straddle each threshold; the grids are the literal values of the formulas.
* The index matrices of the GPU cases hold what the cases rely on: shadow entries, an empty support, a crowded one, list
  lengths 0 ... 9.
"""
import itertools

import numpy as np
import pytest
import torch

import test_pool_branches_gpu as PB
from conftest import golden
from oracle import kpconv_ref
from oracle import pool_ref as P

F32 = np.float32


def _torch_pools(x, inds, dy, fn):
    xt = torch.from_numpy(x).double().requires_grad_(True)
    out = fn(xt, torch.from_numpy(inds))
    out.backward(torch.from_numpy(dy).double())
    return out.detach().numpy(), xt.grad.numpy()


def _tie_case(seed, nq, ns, h, c, lo=-3, hi=4):
    rng = np.random.default_rng(seed)
    inds = PB.make_inds(rng, nq, h, ns)
    x = rng.integers(lo, hi, size=(ns, c)).astype(F32)
    dy = rng.integers(-2, 3, size=(nq, c)).astype(F32)
    return inds, x, dy


def test_max_pool_ref_agrees_with_torch_on_ties():
    for seed, (nq, ns, h, c, lo, hi) in enumerate([(40, 30, 7, 12, -3, 4), (40, 30, 7, 12, -3, 0), (1, 5, 1, 3, -3, 4),
                                                   (9, 2, 21, 5, -1, 2), (64, 300, 255, 4, -3, 4)]):
        inds, x, dy = _tie_case(seed, nq, ns, h, c, lo, hi)
        out, arg = P.max_pool_ref(x, inds)
        vals = np.concatenate([x, np.zeros((1, c), F32)])[inds]
        assert ((vals == out[:, None, :]).sum(1) > 1).mean() > 0.3 or h == 1      # the data is tie-heavy
        t_out, t_dx = _torch_pools(x, inds, dy, kpconv_ref.max_pool_ref)
        assert np.array_equal(out, t_out)
        # arg names a column that attains the maximum, and no earlier one does
        q, ch = np.indices(arg.shape)
        assert np.array_equal(vals[q, arg, ch], out)
        earlier = np.arange(h)[None, :, None] < arg[:, None, :]
        assert not ((vals == out[:, None, :]) & earlier).any()
        dx, n, sabs = P.max_pool_bwd_ref(dy, arg, inds, ns)
        assert np.array_equal(dx, t_dx)                        # torch's CPU max routes to the first maximum too
        assert n.sum() == ((inds[q, arg] < ns)).sum() and np.all(sabs >= np.abs(dx))
        add = np.random.default_rng(99).integers(-2, 3, size=dx.shape).astype(F32)
        dxa, na, sa = P.max_pool_bwd_ref(dy, arg, inds, ns, add)
        assert np.array_equal(dxa, dx + add) and np.array_equal(na, n) and np.array_equal(sa, sabs + np.abs(add))


def test_negative_rows_lose_to_the_shadow_row():
    inds, x, dy = _tie_case(7, 30, 20, 5, 8, -3, 0)
    out, arg = P.max_pool_ref(x, inds)
    has_shadow = (inds == 20).any(1)
    assert has_shadow.any() and not has_shadow.all()
    assert (out[has_shadow] == 0).all() and (out[~has_shadow] < 0).all()
    first_shadow = (inds == 20).argmax(1)
    assert np.array_equal(arg[has_shadow], np.broadcast_to(first_shadow[has_shadow, None], arg[has_shadow].shape))
    dx, n, _ = P.max_pool_bwd_ref(dy, arg, inds, 20)
    assert n.sum() == (~has_shadow).sum() * 8                  # a shadow winner carries no gradient anywhere


def test_closest_pool_ref_agrees_with_torch():
    inds, x, dy = _tie_case(3, 50, 17, 4, 6)
    inds[:4, 0] = 17
    t_out, t_dx = _torch_pools(x, inds, dy, kpconv_ref.closest_pool_ref)
    assert np.array_equal(P.closest_pool_ref(x, inds), t_out)
    dx, n, sabs = P.closest_pool_bwd_ref(dy, inds, 17)
    assert np.array_equal(dx, t_dx)
    assert np.array_equal(n[:, 0], np.bincount(inds[:, 0], minlength=18)[:17]) and np.all(sabs >= np.abs(dx))


def test_refs_agree_with_g6():
    g = golden("g6_pools.npz")
    x, inds, dy = g["x"], g["inds"].astype(np.int64), g["dy"]
    out, arg = P.max_pool_ref(x, inds)
    assert np.array_equal(out, g["max_pool"])
    dx, n, sabs = P.max_pool_bwd_ref(dy, arg, inds, x.shape[0])
    assert not P.violations(g["grad_max_pool"], dx, P.bwd_bound(n, sabs, dx)).any()
    xc, up, dyc = g["xc"], g["up"].astype(np.int64), g["dyc"]
    assert np.array_equal(P.closest_pool_ref(xc, up), g["closest_pool"])
    dxc, n, sabs = P.closest_pool_bwd_ref(dyc, up, xc.shape[0])
    assert not P.violations(g["grad_closest_pool"], dxc, P.bwd_bound(n, sabs, dxc)).any()


def test_bound_passes_f32_sums_and_flags_a_lost_or_doubled_term():
    rng = np.random.default_rng(5)
    nq, ns, h, c = 300, 12, 6, 8
    inds = PB.make_inds(rng, nq, h, ns)
    x = rng.standard_normal((ns, c)).astype(F32)
    dy = (rng.standard_normal((nq, c)) * np.exp(rng.normal(0, 2, size=(nq, 1)))).astype(F32)
    _, arg = P.max_pool_ref(x, inds)
    ref, n, sabs = P.max_pool_bwd_ref(dy, arg, inds, ns)
    tol = P.bwd_bound(n, sabs, ref)

    def f32_sums(skip=None, twice=None):
        dx = np.zeros((ns, c), F32)
        for p in range(nq * h):
            q, col = divmod(p, h)
            s = inds[q, col]
            if s < ns and p != skip:
                m = arg[q] == col
                dx[s, m] += dy[q, m] * (2 if p == twice else 1)
        return dx

    assert not P.violations(f32_sums(), ref, tol).any()
    live = [p for p in range(nq * h) if inds[p // h, p % h] < ns and (arg[p // h] == p % h).any()]
    assert P.violations(f32_sums(skip=live[len(live) // 2]), ref, tol).any()
    assert P.violations(f32_sums(twice=live[len(live) // 3]), ref, tol).any()
    assert P.violations(np.full_like(ref, np.nan), ref, tol).all()
    assert P.describe(f32_sums(skip=live[0]), ref, tol, "dx").startswith("dx: ")


def test_transposed_table_ref_against_nonzero():
    rng = np.random.default_rng(11)
    for nq, h, ns in ((0, 3, 4), (1, 1, 1), (37, 5, 9), (200, 16, 3), (50, 4, 0)):
        inds = rng.integers(-1, ns + 2, size=(nq, h)).astype(np.int64)       # -1 and ns + 1: shadow like ns
        off, pairs = P.transposed_table_ref(inds, ns)
        assert off.shape == (ns + 2,) and off[0] == 0
        flat = inds.reshape(-1)
        for s in range(ns):
            assert np.array_equal(pairs[off[s]:off[s + 1]], np.nonzero(flat == s)[0])
        assert off[ns] == off[ns + 1] == pairs.size == ((flat >= 0) & (flat < ns)).sum()


# ------------------------------------------------------------------------------------------------------------------
# the case tables cover the plans (ws_pool_variant: PB.variant)
# ------------------------------------------------------------------------------------------------------------------
SWEEP_C = (1, 4, 5, 16, 20, 30, 32, 36, 64, 68, 96, 128, 130, 132, 256, 260, 512, 1024)
SWEEP_ROWS = (1, 8191, 8192, 20000)


def sweep_plans():
    """every name the reporter gives over the product; misaligned rows sit where the GPU tables' shift puts them (4 bytes
    off for f32, 2 for bf16)"""
    plans = set()
    for flag in (1, 0):
        with PB.closest_vec_switch(flag):
            for op, d, c, rows, al, o, ab in itertools.product(PB.POOL_OPS, ("f32", "bf16"), SWEEP_C, SWEEP_ROWS, (True, False),
                                                               (False, True), (4, 1)):
                if ab == 1 and (not op.startswith("max") or d != "f32" or c % 4 or not al):
                    continue                                   # the byte forms' preconditions (their caller checks them)
                plans.add(PB.variant(op, d, c, rows, *PB.fake_rows(d, 0 if al else 1), PB.FAKE_ARG, ab, o)[0])
    return plans


def _field(name, key):
    """the integer after `key` in a reporter name ('G=', 'split=')"""
    return int(name.split(key)[1].split()[0])


def test_reporter_refuses_what_no_entry_takes():
    """the byte record outside its preconditions, an unknown operation, an unknown record width: refused, nothing named"""
    from weasal_amd import _lib
    a, b = PB.fake_rows("f32")
    for args in (("max_fwd", "f32", 6, 10, a, b, PB.FAKE_ARG, 1), ("max_bwd", "f32", 8, 10, a + 4, b, PB.FAKE_ARG, 1),
                 ("max_fwd", "bf16", 8, 10, a, b, PB.FAKE_ARG, 1), ("closest_fwd", "f32", 8, 10, a, b, PB.FAKE_ARG, 1),
                 ("max_fwd", "f32", 8, 10, a, b, PB.FAKE_ARG, 2)):
        with pytest.raises(_lib.WeasalHipError):
            PB.variant(*args)
    # one operand off its alignment is enough for the generic form; the forward's arg may be NULL
    for op, d in itertools.product(("max_fwd", "max_bwd"), ("f32", "bf16")):
        off = 2 if d == "bf16" else 4
        for da, db, darg in ((off, 0, 0), (0, off, 0), (0, 0, 4), (0, 0, 8)):
            assert PB.variant(op, d, 64, 100, a + da, b + db, PB.FAKE_ARG + darg)[0] == "%s generic %s" % (op, d)
    assert PB.variant("max_fwd", "f32", 64, 100, a, b, None)[0] == "max_fwd vec G=16 U=4 AT=i32 f32 split=1 contiguous"


def test_case_tables_cover_every_plan():
    swept, table = sweep_plans(), PB.case_plans()
    missing = sorted(swept - table)
    print("launch forms reached by the GPU case tables: %d / %d" % (len(swept & table), len(swept)))
    for p in sorted(table):
        print("  " + p)
    assert not missing, "forms the launchers' ladders produce that no GPU case reaches:\n  " + "\n  ".join(missing)
    assert not table - swept, sorted(table - swept)


def test_plan_set_is_the_expected_one():
    """the full set, counted: vec forms G x record x dtype x assignment x split, the generic and the closest forms"""
    table = PB.case_plans()
    vec = [p for p in table if " vec G=" in p and p.startswith("max")]
    for op, gs in (("max_fwd", (4, 8, 16, 32, 64)), ("max_bwd", (8, 16, 32, 64))):
        for g, at, d, asg in itertools.product(gs, ("i32", "u8"), ("f32", "bf16"), ("interleaved", "contiguous")):
            if at == "u8" and d == "bf16":
                continue
            splits = {int(p.split("split=")[1].split()[0]) for p in vec
                      if p.startswith("%s vec G=%d " % (op, g)) and "AT=%s %s " % (at, d) in p and p.endswith(asg)}
            assert splits == ({1, 2, 4} if g == 64 else {1}), (op, g, at, d, asg, splits)
    assert {p for p in vec if "U=8" in p} == {"max_fwd vec G=32 U=8 AT=u8 f32 split=1 %s" % a for a in ("interleaved", "contiguous")}
    rest = table - set(vec)
    assert rest == {"max_fwd generic f32", "max_fwd generic bf16", "max_bwd generic f32", "max_bwd generic bf16",
                    "closest_fwd scalar f32", "closest_fwd scalar bf16", "closest_bwd scalar f32", "closest_bwd scalar bf16",
                    "closest_bwd vec G=8", "closest_bwd vec G=16", "closest_bwd vec G=32", "closest_bwd vec G=64"}


def test_tables_straddle_the_thresholds():
    cs = {r["c"] for r in PB.MAX_ROWS}
    for edge in (16, 32, 64, 128, 256):
        assert edge in cs and min(c for c in cs if c > edge and c % 4 == 0) == edge + 4
    big = [r for r in PB.MAX_ROWS if r["sizes"][0][0] >= 8192]
    assert {r["c"] for r in big if r["c"] > 256} == {260, 512}                # unsplit G = 64, several channel trips

    def splits(r):
        """split= of every max-pool launch of a row of the table, forward and backward"""
        a, b = PB.fake_rows(r["dtype"], r["shift"])
        return {_field(PB.variant(op, r["dtype"], r["c"], rows, a, b, PB.FAKE_ARG)[0], "split=")
                for nq, ns, _h in r["sizes"] for op, rows in (("max_fwd", nq), ("max_bwd", ns))}

    assert all(splits(r) == {1} for r in big)
    wide = [r for r in PB.MAX_ROWS if r["c"] > 256 and r not in big]
    assert set().union(*map(splits, wide)) == {2, 4} and all(1 not in splits(r) for r in wide)
    # the row threshold itself: 8191 rows split, 8192 do not
    for op in ("max_fwd", "max_bwd"):
        assert [_field(PB.variant(op, "f32", 1024, rows, *PB.fake_rows("f32"), PB.FAKE_ARG)[0], "split=")
                for rows in (8191, 8192)] == [4, 1]
        assert [_field(PB.variant(op, "f32", c, 8191, *PB.fake_rows("f32"), PB.FAKE_ARG)[0], "split=")
                for c in (256, 260, 512, 516)] == [1, 2, 2, 3]
    assert any(r["sizes"][0][0] > 4 * 4096 and r["orders"] == (None,) for r in big)      # past the grid cap, contiguous
    assert any(r["sizes"][0][0] > 8192 and "perm" in r["orders"] for r in big)           # several interleaved trips
    assert any(r["shift"] and r["c"] % 4 == 0 for r in PB.MAX_ROWS)
    assert {(r["c"], r["dtype"]) for r in PB.MAX_ROWS if r["c"] % 4} == {(5, "f32"), (5, "bf16"), (30, "f32"), (30, "bf16")}
    for r in PB.MAX_ROWS:
        if r in big:
            continue
        sf = 64 // PB._g("fwd", r["c"])
        assert {1, sf, sf + 1, 7 * sf, 8 * sf + 3} <= {s[0] for s in r["sizes"]}
        assert {1, 3, 4, 5, 8, 9, 21} == {s[2] for s in r["sizes"]}
    u8 = PB.U8_CASES
    assert {16, 32, 64, 128, 256, 512} <= {c for c, *_ in u8}
    assert {3, 8, 9, 59, 255} <= {h for c, _, _, h in u8 if c == 128} and all(nq <= 64 for _, nq, _, h in u8 if h == 255)
    assert set(PB.TABLE_LENGTHS) >= {64, 65, 2048, 2049} and {4094, 4095} <= set(PB.TABLE_NS)
    assert -(-(PB.TABLE_NS_3LEVEL + 2) // 4096) > 4095 and -(-(PB.TABLE_NS_3LEVEL + 1) // 4096) <= 4096


def test_table_lanes_per_row_are_the_reporters():
    """PB._g, which sizes the case tables at import time, is the library's G for every width of MAX_ROWS, forward and
    backward (widths that are no multiple of 4 have no vector form: the reporter names the generic kernel for them)"""
    for d, c in sorted({(r["dtype"], r["c"]) for r in PB.MAX_ROWS}):
        for op in ("fwd", "bwd"):
            name = PB.variant("max_" + op, d, c, 100, *PB.fake_rows(d), PB.FAKE_ARG)[0]
            if c % 4:
                assert name == "max_%s generic %s" % (op, d)
            else:
                assert _field(name, "G=") == PB._g(op, c), (name, c)


def test_grids_are_the_literal_values():
    """workgroups per launch, worked out by hand from the formulas: contiguous = ceil(groups / 4) capped at 4096 and rounded
    up to whole rounds of 8 past 8; interleaved = 8 min(256, ceil(groups / 32)); groups = ceil(rows / (64 / G)) split"""
    a, b = PB.fake_rows("f32")

    def grid(op, c, rows, ordered=False, rows_a=a):
        return PB.variant(op, "f32", c, rows, rows_a, b, PB.FAKE_ARG, ordered=ordered)[1]

    for op in ("max_fwd", "max_bwd"):
        assert (grid(op, 128, 71000, True), grid(op, 128, 71000)) == (2048, 4096)      # G = 32: 35 500 groups
        assert (grid(op, 128, 37, True), grid(op, 128, 37)) == (8, 5)                  # 19 groups
        assert (grid(op, 1024, 11, True), grid(op, 1024, 11)) == (16, 16)              # split 4: 44 groups
        assert (grid(op, 5, 37), grid(op, 5, 37, True)) == (16, 16)                    # generic: a wave per row, no order
        assert grid(op, 64, 37, True, a + 4) == 16                                     # ... on misaligned rows too
    assert grid("max_fwd", 16, 71000, True) == 8 * 139 and grid("max_bwd", 16, 71000, True) == 2048    # G = 4 / 8: 4438 / 8875 groups
    with PB.closest_vec_switch(1):
        assert PB.variant("closest_bwd", "f32", 64, 37, a, b) == ("closest_bwd vec G=16", 16)
    assert PB.variant("closest_fwd", "f32", 64, 37, a, b)[1] == 16 and PB.variant("closest_fwd", "f32", 64, 71000, a, b)[1] == 4096


def test_case_index_matrices_hold_what_the_cases_rely_on():
    for r in PB.MAX_ROWS[:2] + [x for x in PB.MAX_ROWS if x["c"] in (64, 132, 1024) and x["dtype"] == "f32"]:
        for nq, ns, h in r["sizes"]:
            inds = PB.make_inds(PB._rng(r["id"], nq, ns, h), nq, h, ns)
            assert inds.shape == (nq, h) and inds.min() >= 0 and inds.max() <= ns
            if nq * h >= 2:
                assert (inds == ns).any()
            if nq >= 2:
                assert not (inds[1::2] == ns).any()            # rows without a shadow column: only padding could lift them
            lens = np.bincount(inds.reshape(-1), minlength=ns + 1)[:ns]
            if ns >= 3 and nq * h >= 8:
                assert (lens == 0).any() and lens.max() >= min(150, nq * h // 8)
            if (nq, ns, h) == PB.small_sizes(r["c"])[5] or nq >= 8192:
                assert set(range(10)) <= set(lens.tolist()), (r["id"], nq, ns, h)
    for c, _d, _s, h in PB.CLOSEST_BWD:
        inds, ns = PB.closest_ladder_inds(PB._rng("cb", c), c, h)
        s = max(1, 64 // min(c // 4, 64))
        lens = np.bincount(inds[:, 0], minlength=ns + 1)
        assert set(range(2 * s + 2)) <= set(lens[:ns].tolist()) and lens[ns] > 0 and lens[:ns].max() > 2 * s + 1
