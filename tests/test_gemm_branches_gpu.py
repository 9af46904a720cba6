"""Every launch branch of the dense products (weasal_amd/csrc/gemm.hip and its family units gemm_xb.hip / gemm_xty.hip /
gemm_colsum.hip, gemm_bf16.hip) held to a float64 reference, per
element.

`BRANCHES` names, row by row, the entry, the launch plan it must reach and the shape, operand layout and epilogue menu
that reach it.  Before launching, each row's plan is checked against the library's reporters (ws_gemm_xb_variant,
ws_gemm_xty_variant, ws_act_bwd_colsum_variant, ws_gemm_xbt_bf16_variant, ws_act_bwd_colsum_bf16_variant), which call
the dispatchers' own plan functions.  The outputs are checked against oracle/gemm_branch_ref.py: the whole epilogue menu
in float64, the dropout bits replayed in numpy, and a per-element bound from the error model in that module's docstring.

Every output lies in a buffer whose live region starts as NaN (a missed store fails) and whose guard columns (ldy > n)
and guard row (row m) hold a finite sentinel that must come back bit-unchanged.  Rows of x are spread over exp(N(0, 2))
in scale, a few are all zero and must come out exactly as the f32 epilogue of bias + residual.  gemm_xb2 rows run with
both epilogues (ws_gemm_staged 1 and 0) and must agree bit for bit.

The CPU sweep in test_gemm_branches_cpu.py checks that every form the reporters produce over a grid of shapes,
alignments, pitches, scratch budgets and gates is reached by a row here (none is excused at present).
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import priv_abi
from oracle import gemm_branch_ref as R
from weasal_amd import _lib

pytestmark = pytest.mark.gpu

SENT = 7.25
SLOPE = 0.1
DROP_P = 0.3
SEED = 0x1234ABCD5678
BIG_PITCH = 1 << 23         # gemm_xty_kernel: chunk (64) * pitch * 4 >= 2^31; gemm_xb_kernel: 128 * pitch >= 2^29 (pitch 2^22)


def _xb(id, plan, m, k, n, b="rows", x_off=0, ldx=None, ldy=None, bias=True, res=False, ldr=None, rrows=False, act=True,
        gate=None, scratch=None, zero_rows=True, big=0):
    return dict(fam="xb", id=id, plan=plan, m=m, k=k, n=n, b=b, x_off=x_off, ldx=ldx or k, ldy=ldy or n, bias=bias,
                res=res, ldr=ldr or n, rrows=rrows, act=act, gate=gate, scratch=scratch, zero_rows=zero_rows, big=big)


def _xty(id, plan, m, k, n, x_off=0, ldx=None, y_off=0, ldy=None, ldo=0, bf16=False, big=0):
    return dict(fam="xty", id=id, plan=plan, m=m, k=k, n=n, x_off=x_off, ldx=ldx or k, y_off=y_off, ldy=ldy or n, ldo=ldo,
                bf16=bf16, big=big)


def _cs(id, plan, m, n, lddy=None, dy_off=0, y=True, colsum=True, drop=False, bf16=False, dy_f32=True):
    return dict(fam="colsum", id=id, plan=plan, m=m, n=n, lddy=lddy or n, dy_off=dy_off, y=y, colsum=colsum, drop=drop, bf16=bf16,
                dy_f32=dy_f32)


def _xbt(id, plan, m, k, n, out_f32=False, ldy=None, bias=True, res=True, act=True):
    return dict(fam="xbt", id=id, plan=plan, m=m, k=k, n=n, out_f32=out_f32, ldy=ldy or n, bias=bias, res=res, act=act)


def _x2(nt, wn, b="rows", splits=1, csplit=1):
    return "gemm_xb2_kernel<NT=%d, WN=%d> b=%s epilogue=staged splits=%d csplit=%d%s" % (
        nt, wn, b, splits, csplit, " + splitk_epilogue_kernel" if splits > 1 else "")


def _xg(nt, vecx, vecb):
    return "gemm_xb_kernel<NT=%d, BKX=32> vecx=%d vecb=%d" % (nt, vecx, vecb)


def _sh(rows):
    return "gemm_xb_shallow_kernel rows=%d" % rows


def _t2(kt, nt, wk, wn, chunk, chunks, reduce="none", out="flat", t="float"):
    red = {"none": "none", "grouped": "reduce_partials_kernel", "wide": "reduce_partials_wide_kernel"}[reduce]
    return "gemm_xty2_kernel<KT=%d, NT=%d, WK=%d, WN=%d, TI=%s> chunk=%d chunks=%d reduce=%s out=%s" % (kt, nt, wk, wn, t, chunk, chunks,
                                                                                                    red, out)


def _t1(nt, kt, vecx, vecy, chunk=64, chunks=1):
    return "gemm_xty_kernel<NT=%d, KT=%d> vecx=%d vecy=%d chunk=%d chunks=%d reduce=none out=flat" % (nt, kt, vecx, vecy, chunk, chunks)


def _ck(v, chunk, chunks, reduce=True):
    return "act_bwd_colsum_kernel<V=%d> chunk=%d chunks=%d reduce=%s" % (v, chunk, chunks, "reduce_partials_kernel" if reduce else "none")


def _ckb(tg, chunk, chunks, reduce=True):
    return "act_bwd_colsum_bf16_kernel<TG=%s> chunk=%d chunks=%d reduce=%s" % (tg, chunk, chunks,
                                                                             "reduce_partials_bf_kernel" if reduce else "none")


def _xbtp(nt, out_f32, vecout, staged=True):
    return "gemm_xbt_bf16_kernel<NT=%d, OUT_F32=%s> vecout=%d epilogue=%s" % (nt, "true" if out_f32 else "false", vecout,
                                                                           "staged" if staged and vecout else "lanes")


FULL = "full"               # scratch of ws_gemm_xb_scratch_bytes (every split the plan wants)

BRANCHES = [
    # ---- gemm_xb2_kernel<NT, WN>: n at 32 / 33 / 64 / 65, k <= THIN_K, tiles >= 2048 (m 65 504 .. 65 536) -----------
    _xb("xb2_11_n32", _x2(1, 1, csplit=2), 1000, 64, 32, res=True),
    _xb("xb2_12_n33_pad", "refused", 1000, 64, 33),
    _xb("xb2_12_n36", _x2(1, 2, csplit=2), 1000, 64, 36, res=True, ldy=40, gate="y"),
    _xb("xb2_12_n64", _x2(1, 2), 129, 32, 64, gate="mask"),
    _xb("xb2_22_n68", _x2(2, 2, csplit=3), 127, 96, 68, res=True, rrows=True),
    _xb("xb2_22_n128_t", _x2(2, 2, "transposed", csplit=4), 1000, 128, 128, b="t", gate="drop"),
    _xb("xb2_12_n64_t", _x2(1, 2, "transposed", csplit=2), 33, 64, 64, b="t", res=True),
    _xb("xb2_11_n32_t", _x2(1, 1, "transposed"), 31, 32, 32, b="t", gate="y+mask"),
    _xb("xb2_12_pitchedb", _x2(1, 2, csplit=2), 500, 64, 48, b="pitched", res=True, ldy=52),
    _xb("xb2_11_tiles2047", _x2(1, 2), 65504, 32, 64, bias=True, res=True),
    _xb("xb2_21_tiles2048", _x2(2, 1), 65505, 32, 64, res=True, gate="drop"),
    _xb("xb2_21_thin_k", _x2(2, 1, csplit=2), 65536, 64, 128, rrows=True, res=True),
    _xb("xb2_41_deep_k", _x2(4, 1, "transposed", csplit=3), 65536, 96, 128, b="t", gate="y"),
    _xb("xb2_41_n65", _x2(4, 1, csplit=3), 65536, 96, 68, gate="mask", ldy=72),
    _xb("xb2_21_400k", _x2(2, 1, csplit=2), 400000, 64, 64, gate="drop+y", bias=False, act=False),
    # ---- split-K (ws_gemm_xb_scratch_bytes: m < 32768, k >= 512) ------------------------------------------------------
    _xb("split_none_null", _x2(1, 2, csplit=16), 1000, 512, 64, scratch=None),
    _xb("split_full", _x2(1, 2, splits=2, csplit=8) , 1000, 512, 64, scratch=FULL, res=True, rrows=True, gate="drop"),
    _xb("split_full_deep", _x2(2, 2, splits=4, csplit=8), 300, 1024, 128, scratch=FULL, res=True, gate="y+mask"),
    _xb("split_budget_3", _x2(1, 2, splits=3, csplit=11), 33, 1024, 64, scratch=3 * 33 * 64 * 4 + 100, gate="y"),
    _xb("split_budget_1", _x2(1, 2, csplit=32), 33, 1024, 64, scratch=33 * 64 * 4 + 4),
    _xb("split_11", _x2(1, 1, splits=4, csplit=8), 127, 1024, 32, scratch=FULL, res=True, gate="drop"),
    _xb("split_off_m32768", _x2(1, 2, csplit=16), 32768, 512, 64, scratch=1 << 28),
    _xb("split_m32767", _x2(1, 2, csplit=16), 32767, 512, 64, scratch=FULL),
    _xb("split_k511", _xg(2, 0, 1), 1000, 511, 64, scratch=FULL),
    # ---- gemm_xb_shallow_kernel: m >= 4096, k <= 64 and k % 32 != 0, n % 4 == 0, n <= 1024, k n <= 8192 -------------
    _xb("shallow_k1", _sh(64), 4096, 1, 128, res=True),
    _xb("shallow_k3_n4", _sh(2048), 5000, 3, 4, gate="y"),
    _xb("shallow_k9", _sh(128), 8192, 9, 64, rrows=True, res=True),
    _xb("shallow_k45_400k", _sh(256), 400000, 45, 32, gate="drop"),
    _xb("shallow_k63_n128", _sh(64), 4100, 63, 128, gate="y+mask", res=True),
    _xb("shallow_kn8192", _sh(8), 4096, 8, 1024, res=True),
    _xb("shallow_m4095", _xg(2, 0, 1), 4095, 45, 64, gate="y"),
    # ---- gemm_xb_kernel<1|2|4, 32> ------------------------------------------------------------------------------------
    _xb("xbk_unaligned_x", _xg(2, 0, 1), 1000, 64, 64, x_off=1, ldx=64, res=True, gate="y"),
    _xb("xbk_ldx_odd", _xg(1, 0, 1), 129, 32, 32, ldx=33, gate="mask"),
    _xb("xbk_n1", _xg(1, 1, 0), 127, 32, 1, gate="y"),
    _xb("xbk_n3", _xg(1, 1, 0), 33, 64, 3, res=True, ldy=5),
    _xb("xbk_n9", _xg(1, 1, 0), 1000, 32, 9, gate="drop"),
    _xb("xbk_n30", _xg(1, 1, 0), 129, 96, 30, res=True, rrows=True),
    _xb("xbk_n100", _xg(2, 0, 1), 1000, 45, 100, gate="y+mask"),
    _xb("xbk_n300", _xg(4, 0, 1), 500, 150, 300, res=True),
    _xb("xbk_k45_small_m", _xg(2, 0, 1), 1000, 45, 64, gate="drop+y", bias=False, act=False),
    _xb("xbk_k200_n128", _xg(4, 1, 1), 300, 200, 128, gate="y"),
    _xb("xbk_k20_n96", _xg(2, 1, 1), 300, 20, 96, res=True),
    _xb("xbk_n62", _xg(2, 1, 0), 300, 64, 62, res=True),
    _xb("xbk_n130", _xg(4, 1, 0), 129, 128, 130, gate="y"),
    _xb("xbk_scalar_n9", _xg(1, 0, 0), 127, 33, 9, res=True),
    _xb("xbk_k36_n32", _xg(1, 1, 1), 300, 36, 32, res=True, gate="mask"),
    _xb("xbk_scalar_n50", _xg(2, 0, 0), 129, 33, 50, ldy=53, gate="drop"),
    _xb("xbk_big_pitch", _xg(2, 1, 1), 33, 64, 64, ldx=1 << 22, big=1, res=True),
    # ---- edges ---------------------------------------------------------------------------------------------------------
    _xb("edge_m0", "none (m == 0)", 0, 64, 64),
    _xb("edge_m1", _x2(1, 2, csplit=2), 1, 64, 64, res=True, gate="drop"),
    # ---- dW: gemm_xty2_kernel<KT, NT, WK, WN> f32 ----------------------------------------------------------------------
    _xty("t2_1111", _t2(1, 1, 1, 1, 32, 1), 31, 32, 32),
    _xty("t2_1112", _t2(1, 1, 1, 2, 64, 1), 33, 32, 96, y_off=1),
    _xty("t2_1121", _t2(1, 1, 2, 1, 64, 3, "grouped"), 129, 64, 32, x_off=1),
    _xty("t2_1122", _t2(1, 1, 2, 2, 64, 16, "grouped"), 1000, 64, 96, x_off=1, y_off=1),
    _xty("t2_1211", _t2(1, 2, 1, 1, 64, 1), 33, 32, 64),
    _xty("t2_1212", _t2(1, 2, 1, 2, 64, 16, "grouped"), 1000, 32, 128),
    _xty("t2_1221", _t2(1, 2, 2, 1, 64, 16, "grouped"), 1000, 64, 64, x_off=1),
    _xty("t2_1222", _t2(1, 2, 2, 2, 1568, 256, "grouped"), 400000, 96, 96, ldx=97),
    _xty("t2_2111", _t2(2, 1, 1, 1, 64, 1), 33, 64, 32),
    _xty("t2_2112", _t2(2, 1, 1, 2, 64, 16, "grouped"), 1000, 64, 64, y_off=1),
    _xty("t2_2121", _t2(2, 1, 2, 1, 64, 16, "grouped"), 1000, 128, 32),
    _xty("t2_2122", _t2(2, 1, 2, 2, 64, 16, "grouped"), 1000, 128, 96, ldy=97),
    _xty("t2_2211", _t2(2, 2, 1, 1, 64, 2, "grouped"), 127, 64, 64),
    _xty("t2_2212", _t2(2, 2, 1, 2, 64, 16, "grouped"), 1000, 64, 128),
    _xty("t2_2221", _t2(2, 2, 2, 1, 64, 16, "grouped"), 1000, 128, 64),
    _xty("t2_2222_wide", _t2(2, 2, 2, 2, 512, 64, "wide"), 32768, 256, 256),
    _xty("t2_wide_pitched", _t2(2, 2, 2, 2, 224, 36, "wide", "pitched"), 8000, 256, 256, ldo=272),
    _xty("t2_pitched_one", _t2(2, 2, 1, 1, 64, 1, "grouped", "pitched"), 63, 64, 48, ldo=56),
    _xty("t2_pitched_many", _t2(2, 2, 1, 2, 1568, 256, "grouped", "pitched"), 400000, 64, 96, ldo=104),
    _xty("t2_grouped_big", _t2(2, 2, 2, 2, 512, 79, "grouped"), 40000, 256, 256),
    _xty("t2_m32767", _t2(2, 2, 1, 1, 128, 256, "grouped"), 32767, 64, 64),
    _xty("t2_m0", "memset (m == 0) out=flat", 0, 64, 64),
    _xty("t2_m0_pitched", "memset (m == 0) out=pitched", 0, 64, 48, ldo=56),
    _xty("t2_odd_k", _t2(1, 1, 2, 1, 32, 1), 1, 65, 3, ldx=65),
    # ---- dW bf16: gemm_xty2_kernel<..., bf16_t> ------------------------------------------------------------------------
    _xty("b2_1111", _t2(1, 1, 1, 1, 32, 1, t="bf16"), 31, 32, 32, bf16=True),
    _xty("b2_1112", _t2(1, 1, 1, 2, 64, 1, t="bf16"), 33, 32, 96, y_off=1, bf16=True),
    _xty("b2_1121", _t2(1, 1, 2, 1, 64, 3, "grouped", t="bf16"), 129, 64, 32, x_off=1, bf16=True),
    _xty("b2_1122", _t2(1, 1, 2, 2, 64, 16, "grouped", t="bf16"), 1000, 65, 96, ldy=97, bf16=True),
    _xty("b2_1211", _t2(1, 2, 1, 1, 64, 1, t="bf16"), 33, 32, 64, bf16=True),
    _xty("b2_1212", _t2(1, 2, 1, 2, 64, 16, "grouped", t="bf16"), 1000, 32, 128, bf16=True),
    _xty("b2_1221", _t2(1, 2, 2, 1, 64, 16, "grouped", t="bf16"), 1000, 64, 64, ldx=65, bf16=True),
    _xty("b2_1222", _t2(1, 2, 2, 2, 1568, 256, "grouped", t="bf16"), 400000, 96, 96, x_off=1, bf16=True),
    _xty("b2_2111", _t2(2, 1, 1, 1, 64, 1, t="bf16"), 33, 64, 32, bf16=True),
    _xty("b2_2112", _t2(2, 1, 1, 2, 64, 16, "grouped", t="bf16"), 1000, 64, 64, ldy=65, bf16=True),
    _xty("b2_2121", _t2(2, 1, 2, 1, 64, 16, "grouped", t="bf16"), 1000, 128, 32, bf16=True),
    _xty("b2_2122", _t2(2, 1, 2, 2, 64, 16, "grouped", t="bf16"), 1000, 128, 96, ldy=97, bf16=True),
    _xty("b2_2211", _t2(2, 2, 1, 1, 64, 2, "grouped", t="bf16"), 127, 64, 64, bf16=True),
    _xty("b2_2212", _t2(2, 2, 1, 2, 64, 16, "grouped", t="bf16"), 1000, 64, 128, bf16=True),
    _xty("b2_2221", _t2(2, 2, 2, 1, 64, 16, "grouped", t="bf16"), 1000, 128, 64, bf16=True),
    _xty("b2_2222_wide", _t2(2, 2, 2, 2, 512, 64, "wide", t="bf16"), 32768, 256, 256, bf16=True),
    # ---- gemm_xty_kernel<NT, KT>: chunk * max(ldx, ldy) * 4 >= 2^31 (m = 33: one chunk of 64 rows, pitch 2^23) --------
    _xty("t1_11", _t1(1, 1, 1, 1), 33, 32, 32, ldx=BIG_PITCH, big=1),
    _xty("t1_12", _t1(1, 2, 1, 0), 33, 64, 32, ldx=BIG_PITCH, y_off=1, big=1),
    _xty("t1_14", _t1(1, 4, 0, 1), 33, 100, 20, ldx=BIG_PITCH, x_off=1, big=1),
    _xty("t1_21", _t1(2, 1, 1, 1), 33, 20, 64, ldx=BIG_PITCH, big=1),
    _xty("t1_22", _t1(2, 2, 1, 1), 33, 64, 64, ldx=BIG_PITCH, big=1),
    _xty("t1_24", _t1(2, 4, 1, 0), 33, 128, 40, ldx=BIG_PITCH, ldy=41, big=1),
    _xty("t1_41", _t1(4, 1, 1, 1), 33, 32, 128, ldx=BIG_PITCH, big=1),
    _xty("t1_42", _t1(4, 2, 0, 1), 33, 40, 100, ldx=BIG_PITCH, x_off=1, big=1),
    _xty("t1_44", _t1(4, 4, 1, 1), 33, 128, 128, ldx=BIG_PITCH, big=1),
    # ---- act_bwd_colsum_kernel<4|1> ------------------------------------------------------------------------------------
    _cs("cs4_one", _ck(4, 16, 1, False), 1, 64),
    _cs("cs4_many_drop", _ck(4, 16, 63), 1000, 64, lddy=72, drop=True),
    _cs("cs4_400k", _ck(4, 521, 768), 400000, 64, drop=True),
    _cs("cs4_no_y", _ck(4, 16, 9), 129, 128, y=False),
    _cs("cs4_no_colsum", _ck(4, 16, 9, False), 129, 32, colsum=False, drop=True),
    _cs("cs1_odd_n", _ck(1, 16, 3), 33, 30, drop=True),
    _cs("cs1_unaligned", _ck(1, 16, 8), 127, 64, dy_off=1),
    _cs("cs1_wide_n", _ck(1, 16, 63), 1000, 301, y=False),
    _cs("cs_m0", "memset (m == 0)", 0, 64),
    # ---- bf16 -----------------------------------------------------------------------------------------------------------
    _xbt("xbt_1_bf", _xbtp(1, False, 1), 1000, 64, 32),
    _xbt("xbt_1_f32", _xbtp(1, True, 1), 129, 32, 32, out_f32=True),
    _xbt("xbt_2_bf_lanes", _xbtp(2, False, 0), 127, 64, 62, res=False),
    _xbt("xbt_2_f32", _xbtp(2, True, 1), 1000, 96, 64, out_f32=True, ldy=68),
    _xbt("xbt_4_bf", _xbtp(4, False, 1), 33, 128, 128),
    _xbt("xbt_4_f32_lanes", _xbtp(4, True, 0), 1000, 64, 100, out_f32=True, ldy=101),
    _xbt("xbt_1_f32_odd", _xbtp(1, True, 0), 31, 32, 9, out_f32=True, bias=False),
    _xbt("xbt_2_bf_ldy", _xbtp(2, False, 0), 129, 32, 64, ldy=66, res=False),
    _xbt("xbt_1_bf_n9", _xbtp(1, False, 0), 127, 32, 9),
    _xbt("xbt_2_f32_n62", _xbtp(2, True, 0), 33, 64, 62, out_f32=True),
    _xbt("xbt_4_bf_ldy", _xbtp(4, False, 0), 129, 64, 100, ldy=101),
    _xbt("xbt_4_f32", _xbtp(4, True, 1), 300, 128, 128, out_f32=True),
    _xbt("xbt_400k", _xbtp(2, False, 1), 400000, 64, 64),
    _cs("csb_f32", _ckb("float", 128, 8), 1000, 64, bf16=True),
    _cs("csb_bf16", _ckb("bf16", 128, 1, False), 127, 32, bf16=True, dy_f32=False),
    _cs("csb_bf16_many", _ckb("bf16", 521, 768), 400000, 64, bf16=True, dy_f32=False, lddy=68),
    _cs("csb_no_y", _ckb("float", 128, 3), 300, 128, bf16=True, y=False),
]

# gemm_xb2 at n = 33 would need n % 4 == 0: a strided small matrix there must be refused, not computed
REFUSED = [r for r in BRANCHES if r["plan"] == "refused"]


# ------------------------------------------------------------------------------------------------------------------
# layouts: every operand's allocation (elements), pointer offset (elements) and pitch; the reporters see base + offset
# ------------------------------------------------------------------------------------------------------------------
def xb_layout(r):
    m, k, n = r["m"], r["k"], r["n"]
    if r["b"] == "t":
        ldw = ((k + 3) // 4) * 4 + 4
        b = dict(shape=(n, ldw), brs=1, bcs=ldw)
    elif r["b"] == "pitched":
        ldw = n + 12
        b = dict(shape=(k, ldw), brs=ldw, bcs=1)
    else:
        b = dict(shape=(k, n), brs=-1, bcs=1)
    if r["plan"] == "refused":
        b = dict(shape=(n, k), brs=1, bcs=k)
    rn = max(m // 2, 1)
    lay = dict(b=b, rn=rn if r["rrows"] else m, rld=3 if r["rrows"] else 1)
    if r["scratch"] == FULL:
        lay["scratch_bytes"] = max(_lib.lib().ws_gemm_xb_scratch_bytes(m, k, n), 16)
    elif r["scratch"] is None:
        lay["scratch_bytes"] = 0
    else:
        lay["scratch_bytes"] = int(r["scratch"])
    return lay


def gates_of(r):
    g = r["gate"] or ""
    return dict(y="y" in g.split("+"), mask="mask" in g, drop="drop" in g)


def xb_report(r, ptr):
    """reporter string for row r; ptr(name, off) -> address (int) of operand `name` at element offset `off`"""
    lib = _lib.lib()
    lay = xb_layout(r)
    g = gates_of(r)
    buf = C.create_string_buffer(256)
    rc = lib.ws_gemm_xb_variant(ptr("x", r["x_off"]), r["m"], r["k"], r["ldx"], ptr("b", 0), lay["b"]["brs"], lay["b"]["bcs"], r["n"],
                                ptr("bias", 0) if r["bias"] else None, ptr("res", 0) if r["res"] else None, r["ldr"],
                                ptr("gy", 0) if g["y"] else None, r["n"], ptr("mask", 0) if g["mask"] else None, r["n"],
                                ptr("y", 0), r["ldy"], ptr("scratch", 0) if lay["scratch_bytes"] else None, lay["scratch_bytes"],
                                buf, 256)
    return buf.value.decode() if rc == 0 else "refused"


def xty_report(r, ptr):
    lib = _lib.lib()
    buf = C.create_string_buffer(256)
    es = 2 if r["bf16"] else 4
    outp = ptr("out", 4) if r["ldo"] else ptr("out", 0)
    _lib.check(lib.ws_gemm_xty_variant(ptr("x", r["x_off"], es), r["m"], r["k"], r["ldx"], ptr("y", r["y_off"], es), r["n"], r["ldy"], outp,
                                       r["ldo"], ptr("scratch", 0), 1 if r["bf16"] else 0, buf, 256))
    return buf.value.decode()


def cs_report(r, ptr):
    lib = _lib.lib()
    buf = C.create_string_buffer(256)
    if r["bf16"]:
        _lib.check(lib.ws_act_bwd_colsum_bf16_variant(1 if r["dy_f32"] else 0, r["m"], r["n"], ptr("colsum", 0) if r["colsum"] else None,
                                                      ptr("scratch", 0), buf, 256))
    else:
        _lib.check(lib.ws_act_bwd_colsum_variant(ptr("dy", r["dy_off"]), r["m"], r["n"], r["lddy"], ptr("y", 0) if r["y"] else None, r["n"],
                                                 ptr("dz", 0) if r["y"] else None, r["n"], ptr("colsum", 0) if r["colsum"] else None,
                                                 ptr("scratch", 0), buf, 256))
    return buf.value.decode()


def xbt_report(r, ptr):
    lib = _lib.lib()
    buf = C.create_string_buffer(256)
    _lib.check(lib.ws_gemm_xbt_bf16_variant(r["m"], r["k"], r["n"], ptr("bias", 0) if r["bias"] else None,
                                            ptr("res", 0, 2) if r["res"] else None, r["n"], ptr("y", 0, 4 if r["out_f32"] else 2),
                                            r["ldy"], 1 if r["out_f32"] else 0, buf, 256))
    return buf.value.decode()


REPORT = dict(xb=xb_report, xty=xty_report, colsum=cs_report, xbt=xbt_report)


_NAMES = ("x", "b", "bias", "res", "gy", "mask", "y", "scratch", "out", "dy", "dz", "colsum")


def fake_ptr(name, off, es=4):
    """the addresses the GPU run sees, alignment-wise: every allocation at least 256-byte aligned"""
    return 0x10000000 * (1 + _NAMES.index(name)) + off * es


# ------------------------------------------------------------------------------------------------------------------
# GPU side
# ------------------------------------------------------------------------------------------------------------------
DEV = "cuda"


class Flag:
    def __init__(self, name, value):
        self.v = C.c_int.in_dll(_lib.lib(), name)
        self.value = value

    def __enter__(self):
        self.old = self.v.value
        self.v.value = self.value

    def __exit__(self, *a):
        self.v.value = self.old


_BIG = {}


def big_buffer():
    """one 33 x 2^23-float buffer (1.1 GB) shared by the large-pitch rows"""
    if "t" not in _BIG:
        _BIG["t"] = torch.empty(33 * BIG_PITCH + 64, dtype=torch.float32, device=DEV)
    return _BIG["t"]


def _rows_x(rng, m, k, zero_rows):
    x = rng.standard_normal((m, k)) * np.exp(rng.normal(0.0, 2.0, size=(m, 1)))
    zr = np.array([], np.int64)
    if zero_rows and m >= 4:
        zr = np.unique(rng.integers(0, m, size=max(1, min(8, m // 16))))
        x[zr] = 0.0
    return x.astype(np.float32), zr


def _guarded(m, n, ld):
    """(m + 1) x ld output: sentinel everywhere, NaN in the live region"""
    y = torch.full((m + 1, ld), SENT, dtype=torch.float32, device=DEV)
    y[:m, :n] = float("nan")
    return y


def _guard_ok(ybuf, m, n):
    h = ybuf.cpu().numpy().copy()
    h[:m, :n] = SENT
    assert (h.view(np.uint32) == np.float32(SENT).view(np.uint32)).all(), "a guard column / row past the output changed"


def _place(host, ld, off=0, dtype=torch.float32, big=False):
    """device copy of host [rows, cols] with row pitch ld and element offset off; returns (view tensor, base tensor, ptr)"""
    rows, cols = host.shape
    if big:
        base = big_buffer()
        assert off + (rows - 1) * ld + cols <= base.numel()
    else:
        base = torch.zeros(off + max(rows, 1) * ld + 8, dtype=dtype, device=DEV)
    v = base.as_strided((rows, cols), (ld, 1), off)
    v.copy_(torch.from_numpy(np.ascontiguousarray(host)).to(dtype))
    return v, base, base.data_ptr() + off * base.element_size()


def run_xb(r):
    lib = _lib.lib()
    rng = np.random.default_rng(zlib.crc32(r["id"].encode()))
    m, k, n = r["m"], r["k"], r["n"]
    lay = xb_layout(r)
    g = gates_of(r)
    x, zr = _rows_x(rng, m, k, r["zero_rows"])
    bl = rng.standard_normal((k, n)).astype(np.float32) / np.sqrt(k)
    bias = rng.standard_normal(n).astype(np.float32) if r["bias"] else None
    rn = lay["rn"]
    res = rng.standard_normal((rn, n)).astype(np.float32) if r["res"] else None
    rrows = None
    if r["rrows"]:
        idx = rng.integers(0, rn, size=m)
        sp = rng.integers(0, m, size=min(m, 12))
        idx[sp[0::3]] = -1
        idx[sp[1::3]] = rn
        idx[sp[2::3]] = rn + 17
        rrows = np.zeros((m * lay["rld"],), np.int64)
        rrows[::lay["rld"]] = idx
        rrows[1::lay["rld"]] = 999999                                  # between the strided entries: never read
    gy = None
    if g["y"]:
        gy = rng.standard_normal((m, n)).astype(np.float32)
        if gy.size:
            gy.reshape(-1)[rng.integers(0, gy.size, size=min(gy.size, 64))] = 0.0
            gy.reshape(-1)[rng.integers(0, gy.size, size=min(gy.size, 64))] = -0.0
    mask = (rng.random((m, n)) < 0.7).astype(np.uint8) * rng.integers(1, 256, size=(m, n)).astype(np.uint8) if g["mask"] else None
    mscale = float(np.float32(1.0) / np.float32(0.7))
    drop = (DROP_P, SEED, n) if g["drop"] else None

    xdev, _, xp = _place(x, r["ldx"], r["x_off"], big=r["big"] > 0)
    bshape = lay["b"]["shape"]
    bmat = np.zeros(bshape, np.float32)
    if r["b"] == "t" or r["plan"] == "refused":
        bmat[:, :k] = bl.T
    else:
        bmat[:, :n] = bl
    bdev = torch.from_numpy(bmat).to(DEV)
    biasd = torch.from_numpy(bias).to(DEV) if bias is not None else None
    resd = torch.from_numpy(res).to(DEV) if res is not None else None
    rrd = torch.from_numpy(rrows).to(DEV) if rrows is not None else None
    gyd = torch.from_numpy(gy).to(DEV) if gy is not None else None
    mkd = torch.from_numpy(mask).to(DEV) if mask is not None else None
    sb = lay["scratch_bytes"]
    scr = torch.empty(max(sb, 16), dtype=torch.uint8, device=DEV) if sb else None
    P = _lib.ptr
    st = _lib.current_stream()

    def launch(ybuf):
        yp = C.c_void_p(ybuf.data_ptr())
        xv = C.c_void_p(xp)
        common = (xv, m, k, r["ldx"], P(bdev), lay["b"]["brs"], lay["b"]["bcs"], n)
        if g["drop"] and g["y"]:
            assert lay["b"]["brs"] < 0 and not r["bias"] and not r["res"] and not r["act"]
            return lib.ws_gemm_xb_gate_dropout(xv, m, k, r["ldx"], P(bdev), n, P(gyd), n, SLOPE, DROP_P, SEED, yp, r["ldy"], P(scr), sb, st)
        if g["y"] or g["mask"]:
            return lib.ws_gemm_xb_gated_strided(*common, P(biasd), P(resd), r["ldr"], 1 if r["act"] else 0, SLOPE, P(gyd), n, SLOPE,
                                                P(mkd), n, mscale, yp, r["ldy"], P(scr), sb, st)
        if g["drop"] or r["rrows"]:
            f = priv_abi.entry("ws_priv_gemm_xb_ex")
            return f(*common, P(biasd), P(resd), r["ldr"], P(rrd), lay["rld"], rn, 1 if r["act"] else 0, SLOPE,
                     DROP_P if g["drop"] else 0.0, SEED, yp, r["ldy"], P(scr), sb, st)
        return lib.ws_gemm_xb_epilogue_strided(*common, P(biasd), P(resd), r["ldr"], 1 if r["act"] else 0, SLOPE, yp, r["ldy"], P(scr),
                                               sb, st)

    def report(staged):
        def ptr(name, off, es=4):
            t = dict(x=None, b=bdev, bias=biasd, res=resd, gy=gyd, mask=mkd, y=None, scratch=scr)
            if name == "x":
                return xp
            if name == "y":
                return 0x100
            return t[name].data_ptr() + off * es if t[name] is not None else 0
        with Flag("ws_gemm_staged", staged):
            return xb_report(r, ptr)

    if r["plan"] == "refused":
        assert report(1) == "refused"
        ybuf = _guarded(m, n, r["ldy"])
        with pytest.raises(_lib.WeasalHipError, match="strided small matrix"):
            _lib.check(launch(ybuf))
        torch.cuda.synchronize()
        h = ybuf.cpu().numpy()
        assert np.isnan(h[:m, :n]).all(), "a refused launch wrote its output"
        return None
    assert report(1) == r["plan"], (report(1), r["plan"])

    outs = []
    staged_forms = (1, 0) if r["plan"].startswith("gemm_xb2_kernel") else (1,)
    for staged in staged_forms:
        if staged == 0:
            assert report(0) == r["plan"].replace("epilogue=staged", "epilogue=lanes")
        ybuf = _guarded(m, n, r["ldy"])
        with Flag("ws_gemm_staged", staged):
            _lib.check(launch(ybuf))
        torch.cuda.synchronize()
        _guard_ok(ybuf, m, n)
        outs.append(ybuf[:m, :n].cpu().numpy())
    if len(outs) == 2:
        assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), "staged and per-lane epilogues differ"
    got = outs[0]
    if m == 0:
        return 0.0
    resg = R.gathered(res, m, rrows, lay["rld"], rn) if res is not None else None
    gates = dict(act=r["act"], slope=SLOPE, drop=drop, gate_y=gy, gate_slope=SLOPE, mask=mask, mscale=mscale)
    ref = R.xb_ref(x, bl, bias, resg, **gates)
    splits, csplit = 1, None
    if "splits=" in r["plan"]:
        splits = int(r["plan"].split("splits=")[1].split()[0])
        csplit = int(r["plan"].split("csplit=")[1].split()[0])
    tol = R.xb_bound(x, bl, R.xb_chain(k, splits, csplit), bias, resg, **gates)
    msg = R.describe(got, ref, tol, r["id"])
    assert not msg, msg
    if zr.size:
        want = R.xb_zero_rows_f32(bias, resg[zr] if resg is not None else None, n, act=r["act"], slope=SLOPE, drop=drop, gate_y=gy,
                                  gate_slope=SLOPE, mask=mask, mscale=mscale, rows=zr)
        assert np.array_equal(got[zr], want), "%s: an all-zero row of x is not exactly the f32 epilogue of bias + residual" % r["id"]
    return R.worst_ratio(got, ref, tol)


def _bf(a):
    """round to bf16 (what both sides see)"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def run_xty(r):
    lib = _lib.lib()
    rng = np.random.default_rng(zlib.crc32(r["id"].encode()))
    m, k, n = r["m"], r["k"], r["n"]
    dt = torch.bfloat16 if r["bf16"] else torch.float32
    x, _ = _rows_x(rng, m, k, True)
    y = (rng.standard_normal((m, n)) * np.exp(rng.normal(0, 1.0, size=(m, 1)))).astype(np.float32)
    if r["bf16"]:
        x, y = _bf(x), _bf(y)
    xdev, _, xp = _place(x, r["ldx"], r["x_off"], dt, big=r["big"] > 0)
    ydev, _, yp = _place(y, r["ldy"], r["y_off"], dt)
    sb = max(lib.ws_gemm_xty_scratch_bytes(m, k, n), 16)
    scr = torch.empty(sb, dtype=torch.uint8, device=DEV)
    if r["ldo"]:
        obuf = torch.full((k + 1, r["ldo"]), SENT, dtype=torch.float32, device=DEV)
        obuf[:k, 4:4 + n] = float("nan")
        optr = obuf.data_ptr() + 16
    else:
        obuf = torch.full((k * n + 64,), SENT, dtype=torch.float32, device=DEV)
        obuf[:k * n] = float("nan")
        optr = obuf.data_ptr()

    def ptr(name, off, es=4):
        return dict(x=xp - r["x_off"] * es, y=yp - r["y_off"] * es, out=obuf.data_ptr(), scratch=scr.data_ptr())[name] + off * es

    assert xty_report(r, ptr) == r["plan"], (xty_report(r, ptr), r["plan"])
    st = _lib.current_stream()
    V = C.c_void_p
    if r["bf16"]:
        _lib.check(lib.ws_gemm_xty_bf16(V(xp), m, k, r["ldx"], V(yp), n, r["ldy"], V(optr), _lib.ptr(scr), st))
    elif r["ldo"]:
        f = priv_abi.entry("ws_priv_gemm_xty_pitched")
        _lib.check(f(V(xp), m, k, r["ldx"], V(yp), n, r["ldy"], V(optr), r["ldo"], _lib.ptr(scr), st))
    else:
        _lib.check(lib.ws_gemm_xty(V(xp), m, k, r["ldx"], V(yp), n, r["ldy"], V(optr), _lib.ptr(scr), st))
    torch.cuda.synchronize()
    h = obuf.cpu().numpy()
    if r["ldo"]:
        got = h[:k, 4:4 + n].copy()
        h[:k, 4:4 + n] = SENT
    else:
        got = h[:k * n].reshape(k, n).copy()
        h[:k * n] = SENT
    assert (h.view(np.uint32) == np.float32(SENT).view(np.uint32)).all(), "%s: an element outside dW changed" % r["id"]
    ref = R.xty_ref(x, y)
    if m == 0:
        assert (got == 0).all()
        return 0.0
    chunk = int(r["plan"].split("chunk=")[1].split()[0])
    chunks = int(r["plan"].split("chunks=")[1].split()[0])
    tol = R.xty_bound(x, y, chunk, chunks)
    msg = R.describe(got, ref, tol, r["id"])
    assert not msg, msg
    return R.worst_ratio(got, ref, tol)


def run_colsum(r):
    lib = _lib.lib()
    rng = np.random.default_rng(zlib.crc32(r["id"].encode()))
    m, n = r["m"], r["n"]
    bf = r["bf16"]
    dy = (rng.standard_normal((m, n)) * np.exp(rng.normal(0, 2.0, size=(m, 1)))).astype(np.float32)
    yv = rng.standard_normal((m, n)).astype(np.float32)
    if yv.size:
        yv.reshape(-1)[rng.integers(0, yv.size, size=min(yv.size, 32))] = 0.0
        yv.reshape(-1)[rng.integers(0, yv.size, size=min(yv.size, 32))] = -0.0
    if bf:
        yv = _bf(yv)
        if not r["dy_f32"]:
            dy = _bf(dy)
    dyt = torch.float32 if (not bf or r["dy_f32"]) else torch.bfloat16
    rt = torch.bfloat16 if bf else torch.float32
    dyd, _, dyp = _place(dy, r["lddy"], r["dy_off"], dyt)
    yd = torch.from_numpy(yv).to(DEV).to(rt) if r["y"] else None
    dzb = _guarded(m, n, n + 4).to(rt) if (r["y"] or bf) else None
    dzp = dzb.data_ptr() if dzb is not None else None
    csb = torch.full((n + 8,), SENT, dtype=torch.float32, device=DEV) if r["colsum"] else None
    if csb is not None:
        csb[:n] = float("nan")
    sbytes = (lib.ws_act_bwd_colsum_bf16_scratch_bytes if bf else lib.ws_act_bwd_colsum_scratch_bytes)(m, n)
    scr = torch.empty(max(sbytes, 16), dtype=torch.uint8, device=DEV)
    drop = (DROP_P, SEED, n) if r["drop"] else None

    def ptr(name, off, es=4):
        base = dict(dy=dyp - r["dy_off"] * 4, y=yd.data_ptr() if yd is not None else 0, dz=dzp or 0,
                    colsum=csb.data_ptr() if csb is not None else 0, scratch=scr.data_ptr())[name]
        return base + off * es

    assert cs_report(r, ptr) == r["plan"], (cs_report(r, ptr), r["plan"])
    st = _lib.current_stream()
    V = C.c_void_p
    P = _lib.ptr
    ldz = n + 4
    if bf:
        _lib.check(lib.ws_act_bwd_colsum_bf16(V(dyp), 1 if r["dy_f32"] else 0, m, n, r["lddy"], P(yd), n if yd is not None else 0, SLOPE,
                                              V(dzp), ldz, P(csb), P(scr), st))
    elif r["drop"]:
        _lib.check(lib.ws_act_bwd_colsum_dropout(V(dyp), m, n, r["lddy"], P(yd), n, SLOPE, DROP_P, SEED, V(dzp), ldz, P(csb), P(scr), st))
    else:
        _lib.check(lib.ws_act_bwd_colsum(V(dyp), m, n, r["lddy"], P(yd), n, SLOPE, V(dzp) if dzp else None, ldz, P(csb), P(scr), st))
    torch.cuda.synchronize()
    dz_ref, cs_ref = R.colsum_ref(dy, yv if r["y"] else None, SLOPE, drop)
    worst = 0.0
    if m == 0:
        if csb is not None:
            assert (csb[:n].cpu().numpy() == 0).all()
        return 0.0
    tdz, tcs = R.colsum_bounds(dz_ref, int(r["plan"].split("chunk=")[1].split()[0]), int(r["plan"].split("chunks=")[1].split()[0]),
                               bf16_dz=bf)
    if dzb is not None:
        h = dzb.float().cpu().numpy()
        got = h[:m, :n].copy()
        h[:m, :n] = SENT
        assert (h == SENT).all(), "%s: a guard element of dz changed" % r["id"]
        msg = R.describe(got, dz_ref, tdz, r["id"] + " dz")
        assert not msg, msg
        worst = R.worst_ratio(got, dz_ref, tdz)
    if csb is not None:
        h = csb.cpu().numpy()
        assert (h[n:].view(np.uint32) == np.float32(SENT).view(np.uint32)).all()
        msg = R.describe(h[:n], cs_ref, tcs, r["id"] + " colsum")
        assert not msg, msg
        worst = max(worst, R.worst_ratio(h[:n], cs_ref, tcs))
    return worst


def run_xbt(r):
    lib = _lib.lib()
    rng = np.random.default_rng(zlib.crc32(r["id"].encode()))
    m, k, n = r["m"], r["k"], r["n"]
    x = _bf(_rows_x(rng, m, k, False)[0])
    bt = _bf(rng.standard_normal((n, k)).astype(np.float32) / np.sqrt(k))
    bias = rng.standard_normal(n).astype(np.float32) if r["bias"] else None
    res = _bf(rng.standard_normal((m, n)).astype(np.float32)) if r["res"] else None
    xd = torch.from_numpy(x).to(DEV).to(torch.bfloat16)
    btd = torch.from_numpy(bt).to(DEV).to(torch.bfloat16)
    biasd = torch.from_numpy(bias).to(DEV) if bias is not None else None
    resd = torch.from_numpy(res).to(DEV).to(torch.bfloat16) if res is not None else None
    ot = torch.float32 if r["out_f32"] else torch.bfloat16
    outs = []
    for staged in (1, 0):
        ybuf = _guarded(m, n, r["ldy"]).to(ot)

        def ptr(name, off, es=4):
            return dict(bias=biasd.data_ptr() if biasd is not None else 0, res=resd.data_ptr() if resd is not None else 0,
                        y=ybuf.data_ptr())[name] + off * es

        with Flag("ws_gemm_staged", staged):
            want = r["plan"] if staged else r["plan"].replace("epilogue=staged", "epilogue=lanes")
            assert xbt_report(r, ptr) == want, (xbt_report(r, ptr), want)
            _lib.check(lib.ws_gemm_xbt_bf16(_lib.ptr(xd), m, k, k, _lib.ptr(btd), n, k, _lib.ptr(biasd), _lib.ptr(resd), n,
                                            1 if r["act"] else 0, SLOPE, _lib.ptr(ybuf), r["ldy"], 1 if r["out_f32"] else 0,
                                            _lib.current_stream()))
        torch.cuda.synchronize()
        h = ybuf.float().cpu().numpy()
        outs.append(h[:m, :n].copy())
        h[:m, :n] = SENT
        assert (h == SENT).all(), "%s: a guard element changed" % r["id"]
    assert np.array_equal(outs[0], outs[1]), "%s: staged and per-lane epilogues differ" % r["id"]
    got = outs[0]
    ref = R.xb_ref(x, bt.T, bias, res, act=r["act"], slope=SLOPE)
    tol = R.xb_bound(x, bt.T, k, bias, res, ref=ref, bf16_out=not r["out_f32"], act=r["act"], slope=SLOPE)
    msg = R.describe(got, ref, tol, r["id"])
    assert not msg, msg
    return R.worst_ratio(got, ref, tol)


RUN = dict(xb=run_xb, xty=run_xty, colsum=run_colsum, xbt=run_xbt)
WORST = {}


@pytest.mark.parametrize("row", BRANCHES, ids=[r["id"] for r in BRANCHES])
def test_branch(row):
    with Flag("ws_gemm_shallow", 1), Flag("ws_gemm_staged", 1):
        w = RUN[row["fam"]](row)
    if w is not None:
        fam = row["plan"].split("<")[0].split(" ")[0]
        WORST[fam] = max(WORST.get(fam, 0.0), w)
        print("%s: worst |err| / bound %.3g" % (row["id"], w))


def test_dropout_bits_at_row_times_n():
    """The keep bits of the forward epilogue (x = 0 rows: the output is bias * keep * scale), of ws_gemm_xb_gate_dropout and
    of ws_act_bwd_colsum_dropout equal the numpy replay at index row * n + col, with ldy > n (an index built from ldy
    would give other bits)."""
    lib = _lib.lib()
    m, k, n, ldy = 257, 64, 36, 44
    keep = R.drop_keep(SEED, DROP_P, m, n, n)
    assert not np.array_equal(keep, R.drop_keep(SEED, DROP_P, m, n, ldy))
    scale = R.drop_args(DROP_P)[1]
    st = _lib.current_stream()
    P = _lib.ptr
    x = torch.zeros(m, k, device=DEV)
    b = torch.randn(k, n, device=DEV)
    bias = torch.ones(n, device=DEV)
    f = priv_abi.entry("ws_priv_gemm_xb_ex")
    y = torch.full((m, ldy), SENT, device=DEV)
    _lib.check(f(P(x), m, k, k, P(b), -1, 1, n, P(bias), None, 0, None, 1, 0, 0, 0.0, DROP_P, SEED, P(y), ldy, None, 0, st))
    ones = torch.ones(m, k, device=DEV)
    eye = torch.zeros(k, n, device=DEV)
    eye[0, :] = 1.0                                        # x @ eye = 1 everywhere
    g = torch.full((m, ldy), SENT, device=DEV)
    _lib.check(lib.ws_gemm_xb_gate_dropout(P(ones), m, k, k, P(eye), n, None, 0, SLOPE, DROP_P, SEED, P(g), ldy, None, 0, st))
    dy = torch.ones(m, ldy, device=DEV)
    yy = torch.ones(m, ldy, device=DEV)
    dz = torch.full((m, ldy), SENT, device=DEV)
    _lib.check(lib.ws_act_bwd_colsum_dropout(P(dy), m, n, ldy, P(yy), ldy, SLOPE, DROP_P, SEED, P(dz), ldy, None, None, st))
    torch.cuda.synchronize()
    want = np.where(keep, np.float32(scale), np.float32(0.0))
    for name, t in (("forward epilogue", y), ("ws_gemm_xb_gate_dropout", g), ("ws_act_bwd_colsum_dropout", dz)):
        h = t.cpu().numpy()
        assert np.array_equal(h[:, :n], want), "%s: keep bits differ from the replay at row * n + col" % name
        assert (h[:, n:] == SENT).all()


def test_report_worst_ratios():
    """(runs after the table) the worst |err| / bound per kernel family, for the record"""
    for fam, w in sorted(WORST.items()):
        print("worst |err| / bound  %-32s %.3g" % (fam, w))
        assert w <= 1.0
