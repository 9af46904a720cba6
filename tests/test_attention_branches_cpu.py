"""CPU (no GPU needed): what the attention launch-branch tables (tests/att_branch_ref.py) reach, and that the bound of
tests/test_attention_branches_gpu.py has teeth.

* Every row's claimed launch equals what the restated rules give; SPATIAL_ROWS reaches every (NST, CT) instantiation of
  sphere_att_pv_kernel, every output-tile masking of sphere_att_dqk_kernel, 1 - 5 and 7 dv slices, every kind of dv chunk
  walk, every (NST, CT) on the 64-sphere cap, among empty spheres, in the `ramp` and in the `peaked` regime, every NST on
  eleven tiles; CHANNEL_ROWS reaches both backward forms with both signs and every softmax lane layout.
* The dense products of the channel form, asked of the library's reporters (ws_gemm_xty_variant, ws_gemm_xb_variant) per
  sphere the way attention.hip fills them (k = n = ld = c, b strides (-1, 1) or (1, c)) with stand-in addresses.  The forms
  the channel rows reach (chunk / csplit numbers dropped, chunks as 1 or >1):

      xty   memset (m == 0) out=flat
            gemm_xty2_kernel<KT=1, NT=1, WK=1, WN=1, TI=float>   chunks=1 reduce=none | chunks>1 reduce=reduce_partials_kernel
            gemm_xty2_kernel<KT=2, NT=2, WK=1, WN=1, TI=float>   chunks=1 reduce=none | chunks>1 reduce=reduce_partials_kernel
            gemm_xty2_kernel<KT=2, NT=2, WK=2, WN=2, TI=float>   chunks=1 reduce=none | chunks>1 reduce=reduce_partials_kernel
                                                                 | chunks>1 reduce=reduce_partials_wide_kernel
      xb    none (m == 0)
            gemm_xb_kernel<NT=1 | 2 | 4, BKX=32> vecx=1 vecb=1                          (c % 32 != 0: rows only)
            gemm_xb2_kernel<NT=1, WN=1 | NT=1, WN=2 | NT=2, WN=2> b=rows | b=transposed, epilogue=staged splits=1   (c % 32 == 0)

  A sweep of the reporters over every c % 4 == 0, c <= 512 and every m <= 700 finds no other form: c = 32 and c = 132 were
  added to CHANNEL_ROWS for gemm_xb2_kernel<NT=1, WN=1> and gemm_xb_kernel<NT=4>, which the widths of the issue miss.
  Named, not reached: none.
* Teeth: each of the eleven wrong references of att_branch_ref (one defect each) is rejected by the GPU test's bound in at
  least one tensor, on every row it applies to with at most 400 stacked rows; att_ref in float32 is accepted.
* n = 2^22 stacked rows is WS_ERR_UNSUPPORTED from both sphere entries, with no device.
"""
import ctypes as C
import re

import pytest
import torch

import att_branch_ref as R
import att_ref

NST_CT = {(nst, ct) for nst in (2, 8, 16) for ct in (4, 8)}


def _pairs(rows):
    return {(r["nst"], r["ct"]) for r in rows}


def test_rows_claim_what_the_rules_give():
    ids = [r["id"] for r in R.SPATIAL_ROWS] + [r["id"] for r in R.CHANNEL_ROWS]
    assert len(set(ids)) == len(ids)
    assert 25 <= len(R.SPATIAL_ROWS) <= 30
    for r in R.SPATIAL_ROWS:
        assert (r["nst"], r["ct"], r["slices"], r["ot"], r["walk"]) == R.spatial_launch(r["dq"], r["dv"]), r["id"]
        assert r["dq"] % 8 == 0 and r["dq"] <= 64 and r["dv"] % 64 == 0 and r["dv"] <= 512
        assert sum(r["walk"]) == r["dv"] and r["slices"] * 16 * r["ct"] == r["dv"] and 4 * r["nst"] >= r["dq"]
        assert r["set"] in R.LENGTH_SETS and r["regime"] in R.REGIMES
    for r in R.CHANNEL_ROWS:
        assert (r["strided"], r["lanes"]) == (R.channel_strided(r["c"]), R.lane_class(r["c"])), r["id"]
        assert r["c"] % 4 == 0 and r["c"] <= 512
    assert all(len(v) <= R.MAX_SPHERES for v in R.LENGTH_SETS.values())


def test_length_sets_are_the_structures_they_are_meant_to_be():
    e = R.LENGTH_SETS["empties"]
    assert e[0] == 0 and e[-1] == 0 and any(a == 0 and b == 0 for a, b in zip(e, e[1:]))       # leading, trailing, consecutive
    assert 2 * R.TILE in e and any(R.tiles_of(n) == 5 and n % R.TILE == 1 for n in e)
    cap = R.LENGTH_SETS["cap"]
    assert len(cap) == R.MAX_SPHERES and cap[0] == 0 and cap.count(0) == 1 and max(cap) == 70
    assert [R.tiles_of(n) for n in R.LENGTH_SETS["tall"]] == [11] and 700 % R.TILE == 60
    assert max(R.tiles_of(n) for n in R.LENGTH_SETS["edges"]) == 3


def test_spatial_rows_reach_every_launch_branch():
    rows = R.SPATIAL_ROWS
    assert _pairs(rows) == NST_CT
    assert {(16, 64), (24, 128), (32, 192), (40, 320), (48, 64), (56, 448), (64, 384), (64, 512), (8, 64), (8, 128), (8, 192),
            (32, 256)} == {(r["dq"], r["dv"]) for r in rows}
    # output tiles of the dQ / dK kernel: stored in part (dq = 24, 40, 56) and not at all (dq = 16, 48), per NST that has them
    assert R.ot_mask(8) == {"partial"} and R.ot_of(8) == 1                  # NST = 2 has dq = 8 alone: its one tile, half stored
    for nst, partial, masked in ((8, (24,), (16,)), (16, (40, 56), (48,))):
        for dq in partial:
            assert R.nst_of(dq) == nst and "partial" in R.ot_mask(dq) and any(r["dq"] == dq for r in rows)
        for dq in masked:
            assert R.nst_of(dq) == nst and "masked" in R.ot_mask(dq) and "partial" not in R.ot_mask(dq)
            assert any(r["dq"] == dq for r in rows)
    assert {r["slices"] for r in rows} >= {1, 2, 3, 4, 5, 7}
    walks = {r["walk"] for r in rows}
    assert walks >= {(64,), (128,), (128, 64), (128, 128, 64)} and any(len(w) >= 4 for w in walks)
    for lset in ("cap", "empties"):
        assert _pairs(r for r in rows if r["set"] == lset) == NST_CT, lset
    assert {r["nst"] for r in rows if r["set"] == "tall"} == {2, 8, 16}
    for regime in ("ramp", "peaked"):
        assert _pairs(r for r in rows if r["regime"] == regime) == NST_CT, regime
    assert any(r["regime"] == "mild" for r in rows)


def test_channel_rows_reach_every_launch_branch():
    rows = R.CHANNEL_ROWS
    assert {(r["strided"], r["max_minus"]) for r in rows} == {(s, m) for s in (True, False) for m in (True, False)}
    assert {r["lanes"] for r in rows} >= {"1 idle", "1", "2 partial", "8"}
    assert any(r["c"] > 64 and not r["strided"] for r in rows)
    want = {(c, mm, "edges") for c in (4, 12, 36, 64, 96, 100, 256, 512) for mm in (True, False)}
    want |= {(c, "cap") for c in (12, 64, 100)} | {(c, "empties") for c in (36, 96)}
    have = {(r["c"], r["max_minus"], r["set"]) for r in rows if r["kind"] == "channel"}
    have |= {(r["c"], r["set"]) for r in rows if r["kind"] == "channel"}
    assert want <= have
    assert [(r["c"], r["set"]) for r in rows if r["kind"] == "elevation"] == [(96, "edges")]


# ---- the dense products of the channel form -----------------------------------------------------------------------------------
_BASE = {name: 0x10000000 * (i + 1) for i, name in enumerate(("x1", "x2", "value", "a", "out", "d_out", "d_e", "a_t", "d_et", "d_x1",
                                                             "d_x2", "d_value", "scratch"))}


def _addr(name, elems=0):
    """the addresses the GPU run sees, alignment-wise: every allocation at least 256-byte aligned"""
    return C.c_void_p(_BASE[name] + 4 * elems)


def _xty(lib, x, y, out, m, c, row, s):
    buf = C.create_string_buffer(256)
    rc = lib.ws_gemm_xty_variant(_addr(x, row * c), m, c, c, _addr(y, row * c), c, c, C.cast(_addr(out, s * c * c), C.POINTER(C.c_float)),
                                 0, _addr("scratch"), 0, buf, 256)
    assert rc == 0, lib.ws_last_error()
    return buf.value.decode()


def _xb(lib, x, b, y, m, c, row, s, transposed):
    buf = C.create_string_buffer(256)
    f = lambda p: C.cast(p, C.POINTER(C.c_float))
    brs, bcs = (1, c) if transposed else (-1, 1)
    rc = lib.ws_gemm_xb_variant(f(_addr(x, row * c)), m, c, c, f(_addr(b, s * c * c)), brs, bcs, c, None, None, 0, None, 0, None, 0,
                                f(_addr(y, row * c)), c, None, 0, buf, 256)
    assert rc == 0, lib.ws_last_error()
    return buf.value.decode()


def _channel_products(lib, c, lengths):
    """the answers for the per-sphere products of one forward and one backward call, as attention.hip fills them"""
    strided = R.channel_strided(c)
    xty, xb = [], []
    row = 0
    for s, m in enumerate(lengths):
        xty.append(_xty(lib, "x1", "x2", "a", m, c, row, s))                            # E = X1^T X2
        xb.append(_xb(lib, "value", "a", "out", m, c, row, s, False))                   # out = Val A
        xty.append(_xty(lib, "value", "d_out", "d_e", m, c, row, s))                    # dA = Val^T dOut
        xb.append(_xb(lib, "d_out", "a" if strided else "a_t", "d_value", m, c, row, s, strided))      # dVal = dOut A^T
        xb.append(_xb(lib, "x2", "d_e" if strided else "d_et", "d_x1", m, c, row, s, strided))         # dX1 = X2 dE^T
        xb.append(_xb(lib, "x1", "d_e", "d_x2", m, c, row, s, False))                   # dX2 = X1 dE
        row += m
    return xty, xb


def _form(text):
    text = re.sub(r" chunk=\d+", "", text)
    text = re.sub(r"chunks=(\d+)", lambda mt: "chunks=1" if mt.group(1) == "1" else "chunks>1", text)
    return re.sub(r" csplit=\d+", "", text)


def test_channel_rows_reach_every_dense_product_form():
    from weasal_amd import _lib
    lib = _lib.lib()
    reached_xty, reached_xb, mixed_chunks = set(), set(), []
    for r in R.CHANNEL_ROWS:
        xty, xb = _channel_products(lib, r["c"], R.LENGTH_SETS[r["set"]])
        forms = {_form(t) for t in xty}
        if any("chunks=1" in f for f in forms) and any("chunks>1" in f for f in forms):
            mixed_chunks.append(r["id"])
        reached_xty |= forms
        reached_xb |= {_form(t) for t in xb}
    assert any(f.startswith("memset (m == 0)") for f in reached_xty) and "none (m == 0)" in reached_xb
    assert mixed_chunks, "no call with chunks=1 and chunks>1 side by side"
    assert any("b=transposed" in f for f in reached_xb) and any("b=rows" in f for f in reached_xb)
    assert any("reduce_partials_wide_kernel" in f for f in reached_xty) and any("reduce=reduce_partials_kernel" in f for f in reached_xty)
    for kernel in ("gemm_xty2_kernel<KT=1, NT=1, WK=1, WN=1, TI=float>", "gemm_xty2_kernel<KT=2, NT=2, WK=1, WN=1, TI=float>",
                   "gemm_xty2_kernel<KT=2, NT=2, WK=2, WN=2, TI=float>"):
        assert {f for f in reached_xty if f.startswith(kernel)} >= {kernel + " chunks=1 reduce=none out=flat",
                                                                   kernel + " chunks>1 reduce=reduce_partials_kernel out=flat"}
    assert {f.split(" vecx")[0] for f in reached_xb if f.startswith("gemm_xb_kernel")} == {"gemm_xb_kernel<NT=%d, BKX=32>" % nt for nt in (1, 2, 4)}
    xb2 = {(f.split(">")[0] + ">", "transposed" if "b=transposed" in f else "rows") for f in reached_xb if f.startswith("gemm_xb2_kernel")}
    assert xb2 == {("gemm_xb2_kernel<NT=%d, WN=%d>" % p, b) for p in ((1, 1), (1, 2), (2, 2)) for b in ("rows", "transposed")}
    assert not any("splitk" in f for f in reached_xb)                   # (the channel form passes no split-K scratch)
    # everything the reporters can answer for k = n = c <= 512, m <= 700 is reached by a row
    sweep_xty, sweep_xb = set(), set()
    for c in range(4, 516, 4):
        for m in range(0, 701):
            sweep_xty.add(_form(_xty(lib, "x1", "x2", "a", m, c, 0, 0)))
            sweep_xb.add(_form(_xb(lib, "value", "a", "out", m, c, 0, 0, False)))
            if R.channel_strided(c):
                sweep_xb.add(_form(_xb(lib, "d_out", "a", "d_value", m, c, 0, 0, True)))
    assert sweep_xty - reached_xty == set(), sorted(sweep_xty - reached_xty)
    assert sweep_xb - reached_xb == set(), sorted(sweep_xb - reached_xb)


# ---- teeth ---------------------------------------------------------------------------------------------------------------
TEETH_SPATIAL = [r["id"] for r in R.SPATIAL_ROWS if R.ROWS_OF[r["set"]] <= R.TEETH_MAX_ROWS]
TEETH_CHANNEL = [r["id"] for r in R.CHANNEL_ROWS if R.ROWS_OF[r["set"]] <= R.TEETH_MAX_ROWS]


def test_the_forms_by_hand_are_att_ref():
    """with no defect, spatial_manual / channel_manual are the float64 reference: what a defect changes is the defect alone"""
    for rid in TEETH_SPATIAL:
        inputs, r64, _, _ = R.spatial_case(rid)
        got = R.spatial_manual(*inputs[:3], R.LENGTH_SETS[R.SPATIAL_BY_ID[rid]["set"]], *inputs[3:])
        for key, ref in r64.items():
            assert float((got[key] - ref).abs().max()) <= 1e-11 * float(ref.abs().max()), (rid, key)
    for rid in TEETH_CHANNEL:
        row = R.CHANNEL_BY_ID[rid]
        inputs, r64, _, _ = R.channel_case(rid)
        got = R.channel_manual(*inputs[:3], R.LENGTH_SETS[row["set"]], row["max_minus"], inputs[3])
        for key, ref in r64.items():
            assert float((got[key] - ref).abs().max()) <= 1e-11 * float(ref.abs().max()), (rid, key)


def test_the_yardstick_is_finite_and_the_bound_accepts_float32():
    for rows, case in ((R.SPATIAL_ROWS, R.spatial_case), (R.CHANNEL_ROWS, R.channel_case)):
        for r in rows:
            _, r64, err32, r32 = case(r["id"])
            for key, ref in r64.items():
                assert bool(torch.isfinite(ref).all()) and 0.0 < err32[key] < float("inf"), (r["id"], key)
            assert R.violations(r32, r64, err32) == [], r["id"]


def test_the_maximum_rises_where_defect_3_needs_it():
    for r in R.SPATIAL_ROWS:
        if r["regime"] in ("ramp", "peaked") and r["set"] in ("edges", "empties", "tall"):
            q, k = R.spatial_inputs(r["id"])[:2]
            assert R.max_rises(q, k, R.LENGTH_SETS[r["set"]]), r["id"]


@pytest.mark.parametrize("defect", sorted(R.SPATIAL_DEFECTS))
def test_bound_rejects_a_wrong_sphere_attention(defect):
    ran = 0
    for rid in TEETH_SPATIAL:
        row = R.SPATIAL_BY_ID[rid]
        lengths = R.LENGTH_SETS[row["set"]]
        inputs, r64, err32, _ = R.spatial_case(rid)
        if not R.defect_applies(defect, row):
            continue
        if defect == 3 and row["regime"] == "mild" and not R.max_rises(inputs[0], inputs[1], lengths):
            continue
        wrong = R.spatial_manual(*inputs[:3], lengths, *inputs[3:], defect=defect)
        bad = R.violations(wrong, r64, err32)
        print("defect %d %-28s rejected in %s" % (defect, rid, [b[0] for b in bad]))
        assert bad, "the bound accepts defect %d (%s) on %s" % (defect, R.SPATIAL_DEFECTS[defect], rid)
        ran += 1
    assert ran >= 3


@pytest.mark.parametrize("defect", sorted(R.CHANNEL_DEFECTS))
def test_bound_rejects_a_wrong_channel_attention(defect):
    ran = 0
    for rid in TEETH_CHANNEL:
        row = R.CHANNEL_BY_ID[rid]
        if not R.defect_applies(defect, row):
            continue
        inputs, r64, err32, _ = R.channel_case(rid)
        wrong = R.channel_manual(*inputs[:3], R.LENGTH_SETS[row["set"]], row["max_minus"], inputs[3], defect=defect)
        bad = R.violations(wrong, r64, err32)
        print("defect %d %-28s rejected in %s" % (defect, rid, [b[0] for b in bad]))
        assert bad, "the bound accepts defect %d (%s) on %s" % (defect, R.CHANNEL_DEFECTS[defect], rid)
        ran += 1
    assert ran >= 3


# ---- host validation ------------------------------------------------------------------------------------------------------
def test_four_million_stacked_rows_are_refused_without_a_device():
    from weasal_amd import _lib
    lib = _lib.lib()
    null, one = C.c_void_p(None), C.c_void_p(16)           # never dereferenced: validation fails first
    n = 1 << 22
    lens = (C.c_int64 * 1)(n)
    rc = lib.ws_sphere_attention_fwd(one, one, one, n, 8, 64, lens, 1, one, one, null, null)
    assert rc == 2 and b"2^22" in lib.ws_last_error()
    rc = lib.ws_sphere_attention_bwd(one, one, one, one, one, one, null, n, 8, 64, lens, 1, one, one, one, one, 1 << 40, null)
    assert rc == 2 and b"2^22" in lib.ws_last_error()
    two = (C.c_int64 * 2)(n - 1, 1)
    assert lib.ws_sphere_attention_fwd(one, one, one, n, 64, 512, two, 2, one, one, null, null) == 2
