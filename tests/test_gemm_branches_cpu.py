"""CPU side of tests/test_gemm_branches_gpu.py: the per-element bound has teeth, and the branch table covers the dispatch.

* The bounds of oracle/gemm_branch_ref.py pass a correct float32 evaluation and flag each of: one 32-deep k chunk
  dropped, one split-K layer dropped, one row chunk of the dW partials dropped, rows past m entering a dW chunk as
  non-zero, bias added twice on the last partial column quad, a shadow residual row read as row 0, the dropout index
  taken from ldy instead of n, and one row chunk missing from the column sums.
* The reporters (ws_gemm_xb_variant, ws_gemm_xty_variant, ws_act_bwd_colsum_variant, ws_gemm_xbt_bf16_variant,
  ws_act_bwd_colsum_bf16_variant: the dispatchers' own plan functions, no device work) are swept over a grid of shapes,
  alignments, pitches, scratch budgets and gate sets.  Every plan form they produce is reached by a BRANCHES row or
  listed in EXCUSED with its reason.
* The table straddles each threshold of the dispatch, and each row's declared plan is what the reporter says.
"""
import ctypes as C
import itertools
import re

import numpy as np
import pytest

import test_gemm_branches_gpu as GB
from oracle import gemm_branch_ref as R
from weasal_amd import _lib

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------
# the bound has teeth: float32 stand-ins of the kernels' summation structure
# ------------------------------------------------------------------------------------------------------------------
def _xb_case(m=200, k=128, n=36, seed=0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((m, k)) * np.exp(rng.normal(0, 2.0, size=(m, 1)))).astype(F32)
    b = (rng.standard_normal((k, n)) / np.sqrt(k)).astype(F32)
    bias = rng.standard_normal(n).astype(F32)
    return x, b, bias


def _chunked(x, b, drop_chunk=None, splits=1):
    """f32 x @ b as 32-deep chunks added in order (split: `splits` layers of chunks, then the layers in order)"""
    nch = x.shape[1] // 32
    per = -(-nch // splits)
    layers = []
    for z in range(splits):
        acc = np.zeros((x.shape[0], b.shape[1]), F32)
        for c in range(z * per, min(nch, (z + 1) * per)):
            if c == drop_chunk:
                continue
            acc = (acc + x[:, 32 * c:32 * c + 32] @ b[32 * c:32 * c + 32]).astype(F32)
        layers.append(acc)
    return layers


def _sum_layers(layers, skip=None):
    v = np.zeros_like(layers[0])
    for z, l in enumerate(layers):
        if z != skip:
            v = (v + l).astype(F32)
    return v


def _flag(got, ref, tol):
    return int(R.violations(got, ref, tol).sum())


def test_bound_passes_f32_and_flags_a_dropped_k_chunk():
    x, b, bias = _xb_case()
    ref = R.xb_ref(x, b, bias, act=True, slope=0.1)
    tol = R.xb_bound(x, b, R.xb_chain(128), bias, act=True, slope=0.1)
    good = _sum_layers(_chunked(x, b)) + bias
    good = np.where(good > 0, good, good * F32(0.1))
    assert _flag(good, ref, tol) == 0
    bad = _sum_layers(_chunked(x, b, drop_chunk=2)) + bias
    bad = np.where(bad > 0, bad, bad * F32(0.1))
    assert _flag(bad, ref, tol) > 0


def test_bound_flags_a_dropped_split_layer():
    x, b, bias = _xb_case(k=512)
    ref = R.xb_ref(x, b, bias)
    tol = R.xb_bound(x, b, R.xb_chain(512, 4, 4), bias)
    layers = _chunked(x, b, splits=4)
    assert _flag(_sum_layers(layers) + bias, ref, tol) == 0
    assert _flag(_sum_layers(layers, skip=3) + bias, ref, tol) > 0


def test_bound_flags_bias_twice_on_the_last_partial_quad():
    x, b, bias = _xb_case(n=34)
    ref = R.xb_ref(x, b, bias)
    tol = R.xb_bound(x, b, 128, bias)
    got = (x @ b + bias).astype(F32)
    assert _flag(got, ref, tol) == 0
    got[:, 32:] += bias[32:]
    assert _flag(got, ref, tol) > 0


def test_bound_flags_a_shadow_residual_row_read_as_row_0():
    x, b, bias = _xb_case(m=64)
    rng = np.random.default_rng(1)
    rn = 20
    res = rng.standard_normal((rn, 36)).astype(F32)
    idx = rng.integers(0, rn, size=64)
    idx[[3, 9, 17]] = [-1, rn, rn + 5]
    rld = 2
    rrows = np.zeros(64 * rld, np.int64)
    rrows[::rld] = idx
    resg = R.gathered(res, 64, rrows, rld, rn)
    assert (resg[[3, 9, 17]] == 0).all()
    ref = R.xb_ref(x, b, bias, resg)
    tol = R.xb_bound(x, b, 128, bias, resg)
    good = (x @ b + resg.astype(F32) + bias).astype(F32)
    assert _flag(good, ref, tol) == 0
    wrong = resg.copy()
    wrong[[3, 9, 17]] = res[0]
    bad = (x @ b + wrong.astype(F32) + bias).astype(F32)
    assert _flag(bad, ref, tol) > 0


def test_dropout_index_from_ldy_is_flagged():
    m, n, ldy = 50, 36, 44
    x, b, bias = _xb_case(m=m, n=n)
    drop = (GB.DROP_P, GB.SEED, n)
    ref = R.xb_ref(x, b, bias, act=True, drop=drop)
    tol = R.xb_bound(x, b, 128, bias, act=True, drop=drop)
    v = (x @ b + bias).astype(F32)
    v = np.where(v > 0, v, v * F32(0.1))
    _, scale = R.drop_args(GB.DROP_P)
    good = np.where(R.drop_keep(GB.SEED, GB.DROP_P, m, n, n), v * F32(scale), F32(0))
    bad = np.where(R.drop_keep(GB.SEED, GB.DROP_P, m, n, ldy), v * F32(scale), F32(0))
    assert _flag(good, ref, tol) == 0
    assert _flag(bad, ref, tol) > 0


def test_drop_hash_replay_matches_a_scalar_splitmix64():
    """the vectorised replay against a plain-integer transcription of ws_drop_hash"""
    M = (1 << 64) - 1

    def one(seed, i):
        z = (seed + i * 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return (z ^ (z >> 31)) >> 32

    idx = np.array([0, 1, 2, 12345, 2 ** 40 + 7, 2 ** 63 + 11], np.uint64)
    got = R.drop_hash(GB.SEED, idx)
    assert [int(v) for v in got] == [one(GB.SEED, int(i)) for i in idx]
    thr, scale = R.drop_args(0.3)
    assert thr == int(float(np.float32(0.3)) * 2 ** 32) and scale == float(F32(1) / (F32(1) - F32(0.3)))
    assert R.drop_args(np.nextafter(F32(1), F32(0)))[0] <= 2 ** 32 - 1


def _xty_case(m=1000, k=40, n=36, seed=2):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((m, k)) * np.exp(rng.normal(0, 2.0, size=(m, 1)))).astype(F32)
    y = rng.standard_normal((m, n)).astype(F32)
    return x, y


def _xty_f32(x, y, chunk, skip=None, tail_garbage=False):
    m = x.shape[0]
    out = np.zeros((x.shape[1], y.shape[1]), F32)
    for c, a in enumerate(range(0, m, chunk)):
        if c == skip:
            continue
        xs, ys = x[a:a + chunk], y[a:a + chunk]
        if tail_garbage and a + chunk > m:                       # rows past m read as a copy of the last row
            pad = a + chunk - m
            xs = np.concatenate([xs, np.repeat(xs[-1:], pad, 0)])
            ys = np.concatenate([ys, np.repeat(ys[-1:], pad, 0)])
        out = (out + xs.T @ ys).astype(F32)
    return out


def test_bound_flags_dw_chunk_dropped_and_rows_past_m():
    x, y = _xty_case()
    chunk = 96
    chunks = -(-1000 // chunk)
    ref = R.xty_ref(x, y)
    tol = R.xty_bound(x, y, chunk, chunks)
    assert _flag(_xty_f32(x, y, chunk), ref, tol) == 0
    assert _flag(_xty_f32(x, y, chunk, skip=4), ref, tol) > 0
    assert _flag(_xty_f32(x, y, chunk, tail_garbage=True), ref, tol) > 0


def test_bound_flags_a_colsum_chunk_missing():
    rng = np.random.default_rng(3)
    m, n = 500, 32
    dy = (rng.standard_normal((m, n)) * np.exp(rng.normal(0, 2.0, size=(m, 1)))).astype(F32)
    yv = rng.standard_normal((m, n)).astype(F32)
    drop = (GB.DROP_P, GB.SEED, n)
    dz_ref, cs_ref = R.colsum_ref(dy, yv, 0.1, drop)
    chunk = 16
    chunks = -(-m // chunk)
    tdz, tcs = R.colsum_bounds(dz_ref, chunk, chunks)
    _, scale = R.drop_args(GB.DROP_P)
    g = np.where(R.drop_keep(GB.SEED, GB.DROP_P, m, n, n), dy * F32(scale), F32(0)).astype(F32)
    dz = np.where(yv > 0, g, g * F32(0.1)).astype(F32)
    assert _flag(dz, dz_ref, tdz) == 0
    parts = [dz[a:a + chunk].sum(0, dtype=F32) for a in range(0, m, chunk)]
    good = np.zeros(n, F32)
    for p in parts:
        good = (good + p).astype(F32)
    assert _flag(good, cs_ref, tcs) == 0
    bad = (good - parts[7]).astype(F32)
    assert _flag(bad, cs_ref, tcs) > 0


# ------------------------------------------------------------------------------------------------------------------
# the table covers the dispatch
# ------------------------------------------------------------------------------------------------------------------
def atoms(plan):
    """the forms a plan string stands for: the kernel instantiation and each runtime form, one atom each"""
    if "(m == 0)" in plan:
        return {plan}
    kern = plan.split(" ")[0]
    kv = dict(re.findall(r"(\w+)=(\S+)", plan.split(">", 1)[1] if ">" in plan else plan))
    if kern.startswith("gemm_xb2_kernel"):
        out = {kern, "%s b=%s" % (kern, kv["b"])}
        if int(kv["splits"]) > 1:
            out.add("%s split-K" % kern)
        return out
    if kern.startswith("gemm_xb_shallow_kernel"):
        return {kern}
    if kern.startswith("gemm_xb_kernel") or kern.startswith("gemm_xbt_bf16_kernel"):
        return {plan}
    if kern.startswith("gemm_xty2_kernel") or kern.startswith("gemm_xty_kernel"):
        t = "bf16" if "TI=bf16" in plan else "float"
        out = {kern, "xty %s reduce=%s out=%s" % (t, kv["reduce"], kv["out"]),
               "xty %s chunks=%s" % (t, "1" if kv["chunks"] == "1" else "many")}
        if kern.startswith("gemm_xty_kernel"):
            out |= {"gemm_xty_kernel vecx=%s" % kv["vecx"], "gemm_xty_kernel vecy=%s" % kv["vecy"]}
        return out
    if kern.startswith("act_bwd_colsum"):
        return {kern, "%s reduce=%s" % (kern.split("<")[0], kv["reduce"]),
                "%s chunks=%s" % (kern.split("<")[0], "1" if kv["chunks"] == "1" else "many")}
    raise AssertionError(plan)


# forms the sweep produces that no row reaches, with the reason
EXCUSED = {}


def _ptr_factory(offs):
    def ptr(name, off, es=4):
        return GB.fake_ptr(name, off + offs.get(name, 0), es)
    return ptr


def sweep_plans():
    plans = set()
    rep = GB.REPORT
    # xb
    for m, k, n, b, xo, ldxp, scr, gate in itertools.product(
            (0, 1, 33, 1000, 4095, 4096, 32767, 32768, 65504, 65505, 400000), (1, 9, 32, 45, 64, 96, 128, 200, 511, 512, 1024),
            (1, 4, 9, 30, 32, 33, 36, 64, 68, 100, 128, 300, 1024), ("rows", "t", "pitched"), (0, 1), (0, 1),
            (None, GB.FULL, 3 * 4 * 64 * 33), (None, "y+mask")):
        r = GB._xb("s", "", m, k, n, b=b, x_off=xo, ldx=k + ldxp, gate=gate, scratch=scr)
        p = rep["xb"](r, GB.fake_ptr)
        if p != "refused":
            plans.add(p)
    # xty (f32, bf16, pitched) and the large-pitch fallback
    for m, k, n, xo, yo, ldxp, ldo, bf in itertools.product(
            (0, 1, 31, 33, 63, 129, 1000, 8000, 32767, 32768, 400000), (1, 3, 32, 33, 64, 65, 96, 128, 256),
            (1, 3, 32, 33, 64, 65, 96, 128, 256), (0, 1), (0, 1), (0, 1), (0, 8), (0, 1)):
        if bf and ldo:
            continue
        r = GB._xty("s", "", m, k, n, x_off=xo, y_off=yo, ldx=k + ldxp, ldo=(n + ldo) if ldo else 0, bf16=bool(bf))
        plans.add(rep["xty"](r, GB.fake_ptr))
    for k, n, xo, yo, ldyp in itertools.product((20, 32, 40, 64, 100, 128), (20, 32, 40, 64, 100, 128), (0, 1), (0, 1), (0, 1)):
        r = GB._xty("s", "", 33, k, n, x_off=xo, y_off=yo, ldx=GB.BIG_PITCH, ldy=n + ldyp)
        plans.add(rep["xty"](r, GB.fake_ptr))
    # column sums
    for m, n, lddyp, dyo, y, cs, bf, f in itertools.product((0, 1, 33, 1000, 400000), (4, 30, 32, 64, 128, 301), (0, 1), (0, 1),
                                                          (0, 1), (0, 1), (0, 1), (0, 1)):
        if bf and (n % 4 or lddyp):
            continue
        r = GB._cs("s", "", m, n, lddy=n + lddyp, dy_off=dyo, y=bool(y), colsum=bool(cs), bf16=bool(bf), dy_f32=bool(f))
        plans.add(rep["colsum"](r, GB.fake_ptr))
    # bf16 product
    for m, n, f, ldyp, bias, res in itertools.product((0, 33, 1000), (9, 32, 62, 64, 100, 128), (0, 1), (0, 1), (0, 1), (0, 1)):
        r = GB._xbt("s", "", m, 64, n, out_f32=bool(f), ldy=n + ldyp, bias=bool(bias), res=bool(res))
        plans.add(rep["xbt"](r, GB.fake_ptr))
    return plans


def test_table_covers_every_plan_form():
    swept = set().union(*(atoms(p) for p in sweep_plans()))
    table = set().union(*(atoms(r["plan"]) for r in GB.BRANCHES if r["plan"] != "refused"))
    missing = sorted(swept - table - set(EXCUSED))
    print("dispatch forms reached by BRANCHES: %d / %d (excused: %d)" % (len(swept & table), len(swept), len(set(EXCUSED) & swept)))
    for a, why in sorted(EXCUSED.items()):
        print("  excused %s: %s" % (a, why))
    assert not missing, "forms the dispatch produces that no BRANCHES row reaches:\n  " + "\n  ".join(missing)
    kinds = {a.split("<")[0] for a in swept if "<" in a}
    for want in ("gemm_xb2_kernel", "gemm_xb_kernel", "gemm_xty2_kernel", "gemm_xty_kernel", "act_bwd_colsum_kernel",
                 "gemm_xbt_bf16_kernel", "act_bwd_colsum_bf16_kernel"):
        assert want in kinds, want


def test_every_row_matches_its_reporter():
    for r in GB.BRANCHES:
        assert GB.REPORT[r["fam"]](r, GB.fake_ptr) == r["plan"], r["id"]


def test_instantiation_counts():
    """all 5 gemm_xb2 forms, 16 + 16 gemm_xty2 instantiations, 9 gemm_xty forms, both colsum widths, 6 xbt forms"""
    inst = {re.match(r"[^<( ]+(<[^>]*>)?", r["plan"]).group(0) for r in GB.BRANCHES}
    count = lambda pre: len({i for i in inst if i.startswith(pre)})
    assert count("gemm_xb2_kernel") == 5
    assert len({i for i in inst if i.startswith("gemm_xty2_kernel") and "TI=float" in i}) == 16
    assert len({i for i in inst if i.startswith("gemm_xty2_kernel") and "TI=bf16" in i}) == 16
    assert count("gemm_xty_kernel") == 9
    assert count("gemm_xb_kernel") == 3
    assert count("act_bwd_colsum_kernel") == 2
    assert count("gemm_xbt_bf16_kernel") == 6
    assert count("act_bwd_colsum_bf16_kernel") == 2


def _rows(fam, **kw):
    return [r for r in GB.BRANCHES if r["fam"] == fam and all(r[a] == v for a, v in kw.items())]


def test_table_straddles_the_thresholds():
    xb2 = [r for r in _rows("xb") if r["plan"].startswith("gemm_xb2")]
    ns = {r["n"] for r in xb2}
    assert 32 in ns and 64 in ns and min(n for n in ns if n > 32) <= 36 and min(n for n in ns if n > 64) <= 68
    assert any(r["n"] == 33 for r in _rows("xb", plan="refused"))
    ms = {r["m"] for r in xb2}
    assert {65504, 65505} <= ms                                         # tiles 2047 / 2048
    thin = [r for r in xb2 if "WN=1" in r["plan"] and r["n"] > 64]
    assert {r["k"] <= 64 for r in thin} == {True, False}               # THIN_K
    split = [r for r in _rows("xb") if r["scratch"] is not None]
    assert {32767, 32768} <= {r["m"] for r in split} and {511, 512} <= {r["k"] for r in split}
    assert any("splits=1 " in r["plan"] for r in split) and any("splitk" in r["plan"] for r in split)
    assert any(r["scratch"] is None and r["k"] >= 512 for r in _rows("xb"))
    budget = [r for r in split if isinstance(r["scratch"], int)]
    assert any("splits=1 " in r["plan"] for r in budget) and any(1 < int(r["plan"].split("splits=")[1].split()[0]) < 16 for r in budget)
    sh = [r for r in _rows("xb") if "shallow" in r["plan"]]
    assert {1, 3, 9, 45, 63} <= {r["k"] for r in sh} and any(r["k"] * r["n"] == 8192 for r in sh)
    assert 4096 in {r["m"] for r in sh} and any(r["m"] == 4095 and "gemm_xb_kernel" in r["plan"] for r in _rows("xb"))
    gen = [r for r in _rows("xb") if r["plan"].startswith("gemm_xb_kernel")]
    assert {1, 3, 9, 30, 100, 300} <= {r["n"] for r in gen}
    assert any(r["x_off"] for r in gen) and any(r["ldx"] % 4 for r in gen) and any(r["big"] for r in gen)
    xty = _rows("xty")
    assert {32767, 32768} <= {r["m"] for r in xty}
    assert any("wide" in r["plan"] for r in xty) and any("reduce_partials_kernel" in r["plan"] and r["k"] * r["n"] >= 65536
                                                          for r in xty)
    pit = [r for r in xty if r["ldo"]]
    assert {"1", "many"} == {"1" if "chunks=1 " in r["plan"] else "many" for r in pit if r["m"]} and any(r["m"] == 0 for r in pit)
    every = {r["m"] for r in GB.BRANCHES}
    assert {0, 1, 31, 33, 127, 129} <= every
    assert any(r["ldy"] > r["n"] for r in _rows("xb"))
    assert any(r["rrows"] for r in _rows("xb")) and any(r["gate"] and "drop" in r["gate"] for r in split)
    for g in ("y", "mask", "drop", "drop+y", "y+mask"):
        assert any(r["gate"] == g for r in xb2), g
    assert {"y", "mask", "drop"} <= set("+".join(r["gate"] or "" for r in sh).split("+"))


def test_scratch_sizes_of_empty_operands():
    """m = 0 is a valid size for every entry; sizing its scratch must not divide by a zero chunk (the dW sizing did: row
    t2_m0 of the GPU table ended the process with SIGFPE)"""
    lib = _lib.lib()
    for k, n in ((1, 1), (64, 64), (256, 300)):
        assert lib.ws_gemm_xty_scratch_bytes(0, k, n) == lib.ws_gemm_xty_scratch_bytes(1, k, n) > 0
        assert lib.ws_act_bwd_colsum_scratch_bytes(0, n) > 0 and lib.ws_act_bwd_colsum_bf16_scratch_bytes(0, n) > 0
        assert lib.ws_gemm_xb_scratch_bytes(0, k, n) == 0
