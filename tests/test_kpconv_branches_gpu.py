"""Every launch branch of the KPConv gather dispatch (weasal_amd/csrc/kpconv.hip) held to a float64 reference, per element.

`BRANCHES` names, row by row, the kernel instantiation a public entry launches and the inputs that reach it; GRID_SLAB /
GRID_WIDE with GRID_PLAN do the same for the table-free backward.  The table is the independent statement; the library's
own statement is ws_kpconv_gather_variant, which formats the plan functions the launchers call (kpconv.hip: fwd_plan,
bwd_x_plan, bwd_geom_plan, bwd_x_grid_plan, bwd_x_gridw_plan).  Before anything is launched here the reporter is asked
with the real device pointers and has to name the row's kernel, every template argument and csplit / ilv
(tests/test_kpconv_branches_cpu.py asks it about every row with stand-in addresses).  The rules behind the rows:
  forward, ci > 4   NT from ci (<=16: 1, <=32: 2, <=64: 4, <=128: 8, else 16); NT = 1 unless ci % NT == 0 and the rows are
                    16-byte aligned; the rigid linear / sum form on fewer than SPLIT_ROWS queries narrows NT to SPLIT_NT and
                    splits a query into csplit items of one channel block each; rows_sorted + rigid linear / sum launches
                    the CUT form (ws_kpconv_gather_fwd_ex); MODE 0 (rigid linear / sum), 1 (anything else), DEF (deformed_kp
                    given).  VECROW is always true: "masked rows" are NT = 1 with lanes past ci masked, several blocks
                    looped in the kernel when csplit = 1.
  forward, ci <= 4  vec4 (ci % 4 == 0 and aligned rows) -> G = 1, VEC, PW = 4; else (f32 only) G = 4, PW = 1.  MODE 0 = linear /
                    sum, rigid; MODE 1 otherwise.
  K4                the transposed table: G from ci (<=4: 1, <=8: 2, <=16: 4, <=32: 8, else 16), MODE 0 = rigid linear / sum,
                    VEC = ci % 4 == 0 and aligned dwf / dx.  Reached whenever the layer has no search grid (queries distinct
                    from the supports, or no PyramidBatch.activate()).
  K6                one template per row type; vec4 (ci % 4 == 0, aligned) is a kernel argument.
  K4G slab / wide   via ops._KPConvGather.backward on a self-query layer of an activated batch: wide when grid.max_count >
                    ops.GRID_NARROW_MAX (rigid linear / sum only); G, MODE, VEC as K4, SORT = ws_kpconv_grid_sorted, NCH from ci
                    (G = 16 only: <=64: 1, <=128: 2, else 4); ilv = GRID_INTERLEAVE when the supports have a point order.
Unreachable through a public entry (so not in the table): kpconv_gather_fwd_mfma_kernel<..., VECROW=false> (never
instantiated: the dispatch always passes VECROW = true and masks NT = 1 rows instead); bf16 rows that are not 8-byte
aligned or have ci % 4 != 0 (the entries refuse them: rows_vec4_or_f32 in every plan).  MODE 2 (the deformable fast path,
ws_kpconv_gather_*_def) has its own table on this harness: DEF_BRANCHES in test_kpconv_def_branches_gpu.py.  Left to another
module: FUSE (the fused forward layer: test_infer_gpu.py).

Inputs: points on a 2^-6 lattice, kernel points 2^-7 off it (oracle/kpconv_branch_ref.py: every squared distance exact
in f32, no decision flips; the setup asserts the extent margin).  Reference: oracle.kpconv_ref.kpconv_gather_ref in
float64 on the same f32 (or bf16-rounded) values, autograd in float64 for dx, d deformed_kp and d modulations.  Bound:
per element, from the error model in oracle/kpconv_branch_ref.py -- never a fraction of the tensor's maximum.

K4G (the table-free backward) is held to the table form, which the rows above hold to float64: bit-identical with the
pairs summed in index order (ws_kpconv_grid_sorted = 1), within twice the per-element summation bound in grid-walk order.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from oracle import kpconv_branch_ref as R

pytestmark = pytest.mark.gpu

K = 15
EXTENT = 0.3            # extent^2 * 2^14 = 1474.56: no squared distance (a multiple of 2^-14) is within 3e-4 of it
RADIUS = 0.75           # rows reach 2.5 extents: many neighbours outside every influence
KP_REACH = 0.7 * EXTENT * 1.5


def _b(id, entry, kernel, targs, ci, nq, h=None, dtype="f32", influence="linear", aggregation="sum", deform=None,
       rows_sorted=False, view="aligned", queries="self", csplit=1, bwd=None, geom=None, straddle=None, rows="radius",
       ties=False, order=False, note=""):
    return dict(id=id, entry=entry, kernel=kernel, targs=targs, ci=ci, nq=nq, h=h, dtype=dtype, influence=influence,
                aggregation=aggregation, deform=deform, rows_sorted=rows_sorted, view=view, queries=queries, csplit=csplit,
                bwd=bwd, geom=geom, straddle=straddle, rows=rows, ties=ties, order=order, note=note)


MF = "kpconv_gather_fwd_mfma_kernel"
VF = "kpconv_gather_fwd_kernel"
K4 = "kpconv_gather_bwd_x_kernel"
K6 = "kpconv_gather_bwd_geom_kernel"
FWD = {"f32": "ws_kpconv_gather_fwd", "bf16": "ws_kpconv_gather_fwd_bf16"}


def _mf(nt, mode, deff, t, cut=False):
    return "NT=%d, MODE=%d, DEF=%s, VECROW=true, T=%s, CUT=%s" % (nt, mode, "true" if deff else "false", t, "true" if cut else "false")


def _vf(g, mode, deff, vec, pw, t):
    return "K=15, G=%d, MODE=%d, DEF=%s, VEC=%s, PW=%d, T=%s" % (g, mode, "true" if deff else "false", "true" if vec else "false", pw, t)


def _k4(g, mode, vec, t):
    return (K4, "K=15, G=%d, MODE=%d, VEC=%s, T=%s" % (g, mode, "true" if vec else "false", t))


def _k6(t, vec):
    return (K6, "K=15, T=%s (vec4=%d)" % (t, 1 if vec else 0))


def _tn(dt):
    return "float" if dt == "f32" else "bf16"


def _k4g(ci):
    return 1 if ci <= 4 else 2 if ci <= 8 else 4 if ci <= 16 else 8 if ci <= 32 else 16


BRANCHES = []
for _dt in ("f32", "bf16"):
    t = _tn(_dt)
    BRANCHES += [
        # ---- K3 on the matrix core, every NT
        _b("k3_nt1_" + _dt, FWD[_dt], MF, _mf(1, 0, False, t), 16, 600),
        _b("k3_nt2_" + _dt, FWD[_dt], MF, _mf(2, 0, False, t), 32, 600, bwd=_k4(8, 0, True, t)),
        _b("k3_nt4_" + _dt, FWD[_dt], MF, _mf(4, 0, False, t), 64, 600),
        _b("k3_nt8_" + _dt, FWD[_dt], MF, _mf(8, 0, False, t), 128, 4096, straddle=("SPLIT_ROWS", "at", 128)),
        _b("k3_nt16_" + _dt, FWD[_dt], MF, _mf(16, 0, False, t), 256, 4096, straddle=("SPLIT_ROWS", "at", 256)),
        # ---- one query below SPLIT_ROWS: SPLIT_NT narrowing + csplit items
        _b("k3_split128_" + _dt, FWD[_dt], MF, _mf(4, 0, False, t), 128, 4095, csplit=2, straddle=("SPLIT_ROWS", "below", 128)),
        _b("k3_split256_" + _dt, FWD[_dt], MF, _mf(4, 0, False, t), 256, 4095, csplit=4, straddle=("SPLIT_ROWS", "below", 256)),
        # ---- ci % nt != 0: nt falls back to 1, partial last block (100 = 6 x 16 + 4, 260 = 16 x 16 + 4)
        _b("k3_ci100_split_" + _dt, FWD[_dt], MF, _mf(1, 0, False, t), 100, 600, csplit=7),
        _b("k3_ci100_loop_" + _dt, FWD[_dt], MF, _mf(1, 0, False, t), 100, 4096, note="7 blocks looped in the kernel"),
        _b("k3_ci260_loop_" + _dt, FWD[_dt], MF, _mf(1, 0, False, t), 260, 4096, note="17 blocks looped in the kernel"),
        # ---- MODE 1 through each influence / aggregation
        _b("k3_gauss_" + _dt, FWD[_dt], MF, _mf(2, 1, False, t), 32, 600, influence="gaussian", bwd=_k4(8, 1, True, t)),
        _b("k3_const_" + _dt, FWD[_dt], MF, _mf(4, 1, False, t), 64, 600, influence="constant"),
        _b("k3_closest_" + _dt, FWD[_dt], MF, _mf(8, 1, False, t), 128, 600, aggregation="closest",
           note="no SPLIT_NT narrowing outside MODE 0"),
        _b("k3_closest_nt16_" + _dt, FWD[_dt], MF, _mf(16, 1, False, t), 256, 300, influence="constant", aggregation="closest"),
        # ---- deformable (generic entries): MODE 1 + DEF, min_d2, K4 MODE 1, K6
        _b("k3_def_" + _dt, FWD[_dt], MF, _mf(2, 1, True, t), 32, 600, deform="def", bwd=_k4(8, 1, True, t), geom=_k6(t, True)),
        _b("k3_defmod_" + _dt, FWD[_dt], MF, _mf(4, 1, True, t), 64, 600, deform="defmod", bwd=_k4(16, 1, True, t),
           geom=_k6(t, True)),
        _b("k3_defmod_ci20_" + _dt, FWD[_dt], MF, _mf(2, 1, True, t), 20, 400, deform="defmod", bwd=_k4(8, 1, True, t),
           geom=_k6(t, True), note="one partial 32-channel block"),
        _b("k3_def_nt8_" + _dt, FWD[_dt], MF, _mf(8, 1, True, t), 128, 300, deform="def"),
        _b("k3_defmod_nt16_" + _dt, FWD[_dt], MF, _mf(16, 1, True, t), 256, 200, deform="defmod"),
    ]
    # ---- rows sorted by distance (CUT) on rows of ops.radius_neighbors: every NT (no narrowing, no csplit)
    BRANCHES += [_b("k3_cut_nt%d_%s" % (_nt, _dt), "ws_kpconv_gather_fwd_ex", MF, _mf(_nt, 0, False, t, cut=True), _ci, 600,
                    rows_sorted=True, rows="search") for _nt, _ci in ((1, 16), (2, 32), (4, 64), (8, 128), (16, 256))]
    BRANCHES += [
        # ---- VALU form, ci <= 4 (bf16: ci % 4 == 0 only)
        _b("valu_ci4_" + _dt, FWD[_dt], VF, _vf(1, 0, False, True, 4, t), 4, 600, bwd=_k4(1, 0, True, t)),
        _b("valu_ci4_gauss_" + _dt, FWD[_dt], VF, _vf(1, 1, False, True, 4, t), 4, 600, influence="gaussian",
           bwd=_k4(1, 1, True, t), note="15 live kernel points per neighbour: the pool overflows, 16-lane sub-chunks"),
        _b("valu_ci4_def_" + _dt, FWD[_dt], VF, _vf(1, 1, True, True, 4, t), 4, 600, deform="defmod", bwd=_k4(1, 1, True, t),
           geom=_k6(t, True)),
        _b("valu_ci4_cut_" + _dt, "ws_kpconv_gather_fwd_ex", VF, _vf(1, 0, False, True, 4, t), 4, 600, rows_sorted=True,
           rows="search", note="g.cut: the pool form stops at the reach of the kernel points"),
    ]
BRANCHES += [
    _b("k3_ci260_split_f32", FWD["f32"], MF, _mf(1, 0, False, "float"), 260, 600, csplit=17),
    # ---- row-offset views (x = flat[1:]: rows 4 bytes off 16-byte alignment; f32 only, bf16 rows must be aligned)
    _b("k3_offset_mode0_f32", FWD["f32"], MF, _mf(1, 0, False, "float"), 64, 4096, view="offset",
       note="NT=4 refused for unaligned rows: NT=1, 4 blocks looped in the kernel"),
    _b("k3_offset_mode1_f32", FWD["f32"], MF, _mf(1, 1, False, "float"), 48, 600, view="offset", influence="gaussian",
       note="NT=1, 3 blocks looped in the kernel"),
    _b("k3_offset_def_f32", FWD["f32"], MF, _mf(1, 1, True, "float"), 40, 400, view="offset", deform="def"),
    # ---- one channel per lane, deformable, bf16 rows (the f32 form: ties_def_f32): the reporter sweep names it
    _b("k3_def_nt1_bf16", FWD["bf16"], MF, _mf(1, 1, True, "bf16"), 16, 400, deform="def"),
    # ---- K6 scalar form (ci % 4 != 0): f32 only
    _b("k3_defmod_ci30_f32", FWD["f32"], MF, _mf(2, 1, True, "float"), 30, 400, deform="defmod", bwd=_k4(8, 1, False, "float"),
       geom=_k6("float", False)),
    # ---- VALU form, f32 only shapes
    _b("valu_ci1_f32", FWD["f32"], VF, _vf(4, 0, False, False, 1, "float"), 1, 600, bwd=_k4(1, 0, False, "float")),
    _b("valu_ci3_f32", FWD["f32"], VF, _vf(4, 0, False, False, 1, "float"), 3, 600, bwd=_k4(1, 0, False, "float")),
    _b("valu_ci3_gauss_f32", FWD["f32"], VF, _vf(4, 1, False, False, 1, "float"), 3, 600, influence="gaussian",
       bwd=_k4(1, 1, False, "float")),
    _b("valu_ci3_def_f32", FWD["f32"], VF, _vf(4, 1, True, False, 1, "float"), 3, 600, deform="defmod",
       bwd=_k4(1, 1, False, "float"), geom=_k6("float", False)),
    _b("valu_ci4_offset_f32", FWD["f32"], VF, _vf(4, 0, False, False, 1, "float"), 4, 600, view="offset"),
    _b("valu_ci4_offset_closest_f32", FWD["f32"], VF, _vf(4, 1, False, False, 1, "float"), 4, 600, view="offset",
       aggregation="closest"),
    _b("valu_ci4_offset_def_f32", FWD["f32"], VF, _vf(4, 1, True, False, 1, "float"), 4, 600, view="offset", deform="def"),
    # ---- closest with exact ties between kernel points (mirrored pairs): the first kernel point wins in K3, K4, K6
    _b("ties_k3_f32", FWD["f32"], MF, _mf(2, 1, False, "float"), 32, 400, influence="constant", aggregation="closest",
       ties=True, bwd=_k4(8, 1, True, "float")),
    _b("ties_valu_f32", FWD["f32"], VF, _vf(4, 1, False, False, 1, "float"), 3, 400, influence="constant",
       aggregation="closest", ties=True, bwd=_k4(1, 1, False, "float")),
    _b("ties_def_f32", FWD["f32"], MF, _mf(1, 1, True, "float"), 16, 400, aggregation="closest", deform="def", ties=True,
       bwd=_k4(4, 1, True, "float"), geom=_k6("float", True)),
    # ---- scheduling hints: a registered point order on the queries and on the supports
    _b("order_f32", FWD["f32"], MF, _mf(2, 0, False, "float"), 32, 600, queries="distinct", order=True,
       bwd=_k4(8, 0, True, "float")),
]
# ---- K4 through the transposed table: G x fast / generic x vec4 / scalar, on rows where one support has several hundred
# incoming pairs and the supports far from every query have none (queries distinct from the supports: no grid)
for _ci in (4, 3, 8, 6, 16, 14, 32, 30, 64, 50):
    _vec = _ci % 4 == 0
    for _mode, _inf in ((0, "linear"), (1, "gaussian")):
        for _dt in ("f32", "bf16") if _vec else ("f32",):
            t = _tn(_dt)
            if _ci <= 4:
                fk, fa = VF, _vf(1 if _vec else 4, _mode, False, _vec, 4 if _vec else 1, t)
            else:
                nt = 1 if _ci <= 16 else 2 if _ci <= 32 else 4
                nt = nt if _ci % nt == 0 else 1
                fk, fa = MF, _mf(nt, _mode, False, t)
            _cs = -(-_ci // (16 * nt)) if (_mode == 0 and _ci > 4 and _ci > 16 * nt) else 1
            BRANCHES.append(_b("k4_g%d_%s_%s_ci%d_%s" % (_k4g(_ci), "fast" if _mode == 0 else "generic", "vec" if _vec else "scalar",
                                                           _ci, _dt), FWD[_dt], fk, fa, _ci, 400, h=40, dtype=_dt, influence=_inf,
                                  queries="hub", csplit=_cs, bwd=_k4(_k4g(_ci), _mode, _vec, t)))
# ---- row widths (a column chunk is 64 neighbours; the pool form pairs two): all-shadow rows, queries distinct from supports
for _h in (1, 63, 64, 65, 129, 200):
    BRANCHES.append(_b("width_h%d_mfma_f32" % _h, FWD["f32"], MF, _mf(2, 0, False, "float"), 32, 300, h=_h, queries="dense",
                       bwd=_k4(8, 0, True, "float")))
    BRANCHES.append(_b("width_h%d_valu_f32" % _h, FWD["f32"], VF, _vf(4, 0, False, False, 1, "float"), 3, 300, h=_h,
                       queries="dense", bwd=_k4(1, 0, False, "float")))
for _h in (65, 200):
    BRANCHES.append(_b("width_h%d_mfma_bf16" % _h, FWD["bf16"], MF, _mf(2, 0, False, "bf16"), 32, 300, h=_h, dtype="bf16",
                       queries="dense", bwd=_k4(8, 0, True, "bf16")))
    BRANCHES.append(_b("width_h%d_valu_bf16" % _h, FWD["bf16"], VF, _vf(1, 0, False, True, 4, "bf16"), 4, 300, h=_h,
                       dtype="bf16", queries="dense", bwd=_k4(1, 0, True, "bf16")))
BRANCHES.append(_b("width_h129_valu_gauss_f32", FWD["f32"], VF, _vf(4, 1, False, False, 1, "float"), 3, 300, h=129,
                   influence="gaussian", queries="dense", bwd=_k4(1, 1, False, "float")))
# dtype of the rows built in the loops above with a fixed "f32"/"bf16" suffix
for _r in BRANCHES:
    if _r["id"].endswith("_bf16"):
        _r["dtype"] = "bf16"

# ---- K4G, the table-free backward on the self-query layers of an activated batch (test_grid_backward_*)
# (bf16 rows need ci % 4 == 0: the entries refuse the others)
GRID_SLAB = [(ci, variant, dt) for ci in (4, 3, 8, 6, 16, 14, 32, 30, 64, 50) for variant in ("rigid", "gaussian-closest", "deformable")
             for dt in (("f32", "bf16") if ci % 4 == 0 else ("f32",))]
GRID_SLAB_LIMITS = [20, 30, 40, 40, 30]          # every row <= ops.GRID_NARROW_MAX: the slab form
GRID_WIDE_LIMITS = [422, 519, 472, 193, 34]      # the config-5 limits: level-0 rows > ops.GRID_NARROW_MAX, the wide form
GRID_WIDE = [(ci, dt) for ci in (4, 3, 8, 6, 16, 14, 32, 30, 64, 50, 128, 98, 256, 198) for dt in (("f32", "bf16") if ci % 4 == 0 else ("f32",))]
# what those cases launch: G per ci, NCH per ci (wide form), MODE per variant, VEC = ci % 4 == 0 (the rows are aligned),
# SORT = ws_kpconv_grid_sorted, ilv = GRID_INTERLEAVE with a point order on the supports and 0 without
GRID_G = {4: 1, 3: 1, 8: 2, 6: 2, 16: 4, 14: 4, 32: 8, 30: 8, 64: 16, 50: 16, 128: 16, 98: 16, 256: 16, 198: 16}
GRID_NCH = {128: 2, 98: 2, 256: 4, 198: 4}
GRID_MODE = {"rigid": 0, "gaussian-closest": 1, "deformable": 1}
GRID_ILV = 512
K4G = "kpconv_gather_bwd_x_grid_kernel"
K4GW = "kpconv_gather_bwd_x_gridw_kernel"


def grid_plan(ci, variant, dt, wide, sort=False, ordered=False):
    """(kernel, template arguments, ilv) the table-free backward launches for a GRID_SLAB / GRID_WIDE case"""
    tb = lambda v: "true" if v else "false"
    if wide:
        targs = "K=15, G=%d, MODE=%d, VEC=%s, NCH=%d, T=%s" % (GRID_G[ci], GRID_MODE[variant], tb(ci % 4 == 0), GRID_NCH.get(ci, 1), _tn(dt))
    else:
        targs = "K=15, G=%d, MODE=%d, VEC=%s, T=%s, SORT=%s" % (GRID_G[ci], GRID_MODE[variant], tb(ci % 4 == 0), _tn(dt), tb(sort))
    return (K4GW if wide else K4G, targs, GRID_ILV if ordered else 0)


# ------------------------------------------------------------------------------------------------------------------
# the library's own statement of a launch: ws_kpconv_gather_variant
# ------------------------------------------------------------------------------------------------------------------
GATHER_OPS = dict(fwd=0, bwd_x=1, bwd_geom=2, bwd_x_grid=3, fwd_def=4, bwd_x_def=5, bwd_x_grid_wide=6, bwd_geom_def=7)


def parse_launch(text):
    """'kernel<A=1, B=x> k=v ...' -> (kernel, {template argument: value}, {key: int})"""
    kernel, _, rest = text.partition("<")
    targs, _, keys = rest.partition(">")
    args = dict(a.strip().split("=") for a in targs.split(","))
    return kernel, args, {k: int(v) for k, v in (kv.split("=") for kv in keys.split())}


def report(op, nq, ns, ci, rows_a, rows_b, dtype="f32", deformed=False, modulated=False, influence="linear", aggregation="sum",
           rows_sorted=False, ordered=False):
    """parse_launch of the reporter's answer for one entry; rows_a / rows_b are addresses (only their alignment counts)"""
    from weasal_amd import _lib, ops
    buf = C.create_string_buffer(256)
    _lib.check(_lib.lib().ws_kpconv_gather_variant(GATHER_OPS[op], nq, ns, ci, rows_a, rows_b, int(deformed), int(modulated),
                                                   ops.INFLUENCE[influence], ops.AGGREGATION[aggregation], int(dtype == "bf16"),
                                                   int(rows_sorted), int(ordered), buf, 256))
    return parse_launch(buf.value.decode())


def fake_ptr(name, off=0, es=4):
    """the addresses the GPU run sees, alignment-wise: every allocation at least 256-byte aligned"""
    return 0x10000000 * (1 + ("x", "wf", "dwf", "dx").index(name)) + off * es


def table_launch(kernel, targs):
    """a (kernel, template arguments) pair of the table in parse_launch form (K6 carries its vec4 argument in the text)"""
    targs, _, vec4 = targs.partition(" (vec4=")
    return (kernel, dict(a.strip().split("=") for a in targs.split(",")), {"vec4": int(vec4[0])} if vec4 else {})


def check_row_plan(row, ptr, nq, ns):
    """the reporter names what the row says it launches: forward kernel, template arguments and csplit; K4 and K6 where the row
    runs them.  ptr(name) -> address of x / wf / dwf / dx; -> the number of launches checked"""
    kw = dict(dtype=row["dtype"], deformed=row["deform"] is not None, modulated=row["deform"] == "defmod",
              influence=row["influence"], aggregation=row["aggregation"])
    kernel, args, keys = report("fwd", nq, ns, row["ci"], ptr("x"), ptr("wf"), rows_sorted=row["rows_sorted"], ordered=row["order"], **kw)
    want = table_launch(row["kernel"], row["targs"])
    assert (kernel, args) == want[:2] and keys["csplit"] == row["csplit"], (row["id"], kernel, args, keys)
    checked = 1
    for key, op, a, b in (("bwd", "bwd_x", "dwf", "dx"), ("geom", "bwd_geom", "x", "dwf")):
        if row[key]:
            kernel, args, keys = report(op, nq, ns, row["ci"], ptr(a), ptr(b), ordered=row["order"], **kw)
            want = table_launch(*row[key])
            assert (kernel, args) == want[:2] and all(keys[k] == v for k, v in want[2].items()), (row["id"], key, kernel, args, keys)
            checked += 1
    return checked


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------
def _half_for(n, target):
    """cube half-size for n lattice points with ~target neighbours within RADIUS"""
    return float((n * 4.0 / 3.0 * np.pi * RADIUS ** 3 / (8.0 * target)) ** (1.0 / 3.0))


def _tie_kernel(rng):
    """7 mirrored pairs (x -> -x) plus one point: a neighbour with n_x = 0 is equidistant from both of a pair"""
    base = R.lattice_kernel(rng, 7, KP_REACH)
    kp = []
    for i, v in enumerate(base):
        m = v.copy()
        m[0] = -v[0]
        kp += [v, m] if i % 2 == 0 else [m, v]
    kp.append(R.lattice_kernel(rng, 1, KP_REACH)[0])
    return np.asarray(kp, np.float32)


def _setup(row, gpu):
    rng = np.random.default_rng(zlib.crc32(row["id"].encode()))
    nq, ci = row["nq"], row["ci"]
    kp = _tie_kernel(rng) if row["ties"] else R.lattice_kernel(rng, K, KP_REACH)
    if row["queries"] == "hub":
        q = R.lattice_cloud(rng, nq, 0.4)
        s = np.concatenate([R.lattice_cloud(rng, 2000, 1.5), np.zeros((1, 3), np.float32)])   # the hub is the last support
        inds = R.brute_rows(q, s[:-1], RADIUS, row["h"] - 1)
        inds[inds == s.shape[0] - 1] = s.shape[0]                 # shadow of the larger set
        inds = np.concatenate([np.full((nq, 1), s.shape[0] - 1, np.int64), inds], 1)
    elif row["queries"] == "dense":
        s = R.lattice_cloud(rng, 2400, 1.25)
        q = R.lattice_cloud(rng, nq, 0.45)
        inds = R.brute_rows(q, s, RADIUS, row["h"])
        inds[::7] = s.shape[0]                                   # rows that are all shadow
    else:
        half = _half_for(nq, 90 if row["rows"] == "search" else 24)
        s = R.lattice_cloud(rng, nq if row["queries"] == "self" else nq + 37, half)
        q = s if row["queries"] == "self" else R.lattice_cloud(rng, nq, half)
        if row["rows"] == "search":
            from weasal_amd import ops
            S = torch.from_numpy(s).to(gpu)
            inds = ops.radius_neighbors(S, S, [len(s)], [len(s)], RADIUS, dtype=torch.int64).cpu().numpy()
        else:
            inds = R.brute_rows(q, s, RADIUS, 40)
            inds[::11, 20:] = s.shape[0]                          # shorter rows
    deformed = mod = None
    if row["deform"]:
        deformed = R.lattice_deformed(rng, kp, nq, 0 if row["ties"] else 0.05)
        if row["deform"] == "defmod":
            mod = rng.uniform(0.25, 1.0, size=(nq, K)).astype(np.float32)
    assert R.extent_margin(q, s, inds, kp, EXTENT, deformed) > 1e-6
    if row["ties"]:
        assert R.closest_tie_count(q, s, inds, kp, deformed) >= 50, "the tie case must hold exact kernel-point ties"
    x = rng.standard_normal((s.shape[0], ci)).astype(np.float32)
    if row["dtype"] == "bf16":
        x = torch.from_numpy(x).bfloat16().float().numpy()
    return dict(q=q, s=s, inds=inds, kp=kp, deformed=deformed, mod=mod, x=x)


def _gpu_x(x, dtype, view, gpu):
    t = torch.from_numpy(x).to(gpu)
    if dtype == "bf16":
        t = t.bfloat16()
    if view == "offset":
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=gpu)
        flat[1:].copy_(t.reshape(-1))
        t = flat[1:].view(x.shape)
        assert t.data_ptr() % 16 != 0 and t.is_contiguous()
    return t


def _check_plan_on_device(row, X, Q, S, dwf, gpu):
    """check_row_plan with the device pointers of this run: x as passed, wf / dx as ops allocates them (torch.empty /
    empty_like), dwf as the contiguous gradient autograd hands over"""
    bufs = dict(x=X, wf=torch.empty((Q.shape[0], K, row["ci"]), dtype=X.dtype, device=gpu), dx=torch.empty_like(X))
    if dwf is not None:
        bufs["dwf"] = torch.from_numpy(dwf).to(gpu).to(X.dtype)
    check_row_plan(row, lambda name: bufs[name].data_ptr(), Q.shape[0], S.shape[0])


def _run(row, d, gpu, dwf=None, dmin=None):
    from weasal_amd import ops
    Q = torch.from_numpy(d["q"]).to(gpu)
    S = Q if row["queries"] == "self" else torch.from_numpy(d["s"]).to(gpu)
    inds = torch.from_numpy(d["inds"]).to(gpu)
    X = _gpu_x(d["x"], row["dtype"], row["view"], gpu)
    _check_plan_on_device(row, X, Q, S, dwf, gpu)
    if dwf is not None:
        X = X.detach().requires_grad_(True)
    kw = {}
    if d["deformed"] is not None:
        kw["deformed_kp"] = torch.from_numpy(d["deformed"]).to(gpu).requires_grad_(dwf is not None)
        kw["want_min_d2"] = True
        if d["mod"] is not None:
            kw["modulations"] = torch.from_numpy(d["mod"]).to(gpu).requires_grad_(dwf is not None)
    wf, mn = ops.kpconv_gather(X, Q, S, inds, torch.from_numpy(d["kp"]).to(gpu), EXTENT, row["influence"], row["aggregation"],
                               rows_sorted=row["rows_sorted"], **kw)
    out = dict(wf=wf.detach().float().cpu().numpy(), min_d2=mn.detach().cpu().numpy() if mn is not None else None)
    if dwf is not None:
        G = torch.from_numpy(dwf).to(gpu).to(wf.dtype)
        if mn is not None:
            torch.autograd.backward([wf, mn], [G, torch.from_numpy(dmin).to(gpu)])
        else:
            wf.backward(G)
        out["dx"] = X.grad.float().cpu().numpy()
        if "deformed_kp" in kw:
            out["d_dkp"] = kw["deformed_kp"].grad.cpu().numpy()
        if "modulations" in kw:
            out["d_mod"] = kw["modulations"].grad.cpu().numpy()
    torch.cuda.synchronize()
    return out


def _check(got, ref, tol, what):
    msg = R.describe(got, ref, tol, what)
    assert not msg, msg


@pytest.mark.parametrize("row", BRANCHES, ids=[r["id"] for r in BRANCHES])
def test_branch_vs_float64(row, gpu):
    from weasal_amd import ops
    ops.clear_batch_hints()
    ops.clear_point_orders()
    d = _setup(row, gpu)
    bf = row["dtype"] == "bf16"
    q, s, inds, kp, dk, md = d["q"], d["s"], d["inds"], d["kp"], d["deformed"], d["mod"]
    tmax = R.gaussian_tmax(q, s, inds, kp, EXTENT, dk) if row["influence"] == "gaussian" else 0.0
    rng = np.random.default_rng(7)
    dwf = dmin = None
    if row["bwd"]:
        dwf = rng.standard_normal((q.shape[0], K, row["ci"])).astype(np.float32)
        if bf:
            dwf = torch.from_numpy(dwf).bfloat16().float().numpy()
        dmin = rng.standard_normal((q.shape[0], K)).astype(np.float32) if dk is not None else None
    try:
        if row["order"]:
            perm_q = torch.from_numpy(np.random.default_rng(3).permutation(q.shape[0]).astype(np.int32)).to(gpu)
            perm_s = torch.from_numpy(np.random.default_rng(4).permutation(s.shape[0]).astype(np.int32)).to(gpu)
            plain = _run(row, d, gpu, dwf, dmin)
        got = None
        if row["order"]:
            # the hint is keyed by the point tensor: register the tensors _run will pass
            from weasal_amd import ops as _ops
            Q = torch.from_numpy(q).to(gpu)
            S = torch.from_numpy(s).to(gpu)
            _ops.register_point_order(Q, perm_q)
            _ops.register_point_order(S, perm_s)
            got = _run_with_points(row, d, gpu, Q, S, dwf, dmin)
            assert _ops._order_for(Q) is not None and _ops._order_for(S) is not None
            for key in plain:
                if plain[key] is not None:
                    assert np.array_equal(plain[key], got[key]), "%s changed under a scheduling order" % key
        else:
            got = _run(row, d, gpu, dwf, dmin)
    finally:
        ops.clear_point_orders()
    ref, ref_min = R.ref_forward(d["x"], q, s, inds, kp, EXTENT, row["influence"], row["aggregation"], dk, md)
    tol = R.fwd_bound(d["x"], q, s, inds, kp, EXTENT, row["influence"], row["aggregation"], dk, md, tmax, ref, bf)
    _check(got["wf"], ref, tol, "wf")
    if dk is not None:
        _check(got["min_d2"], ref_min, 4 * R.U * np.abs(ref_min), "min_d2")
    if not row["bwd"]:
        return
    rdx, rdk, rdm = R.ref_backward(d["x"], dwf, q, s, inds, kp, EXTENT, row["influence"], row["aggregation"], dk, md, dmin)
    tol = R.dx_bound(dwf, q, s, inds, kp, EXTENT, row["influence"], row["aggregation"], dk, md, tmax, rdx, bf, d["x"].shape)
    _check(got["dx"], rdx, tol, "dx")
    if row["queries"] == "hub":
        ns = s.shape[0]
        cnt = np.bincount(inds[inds < ns], minlength=ns)
        assert cnt[ns - 1] >= 300 and (cnt == 0).sum() >= 100, "hub / unreached supports missing"
        assert np.abs(rdx[ns - 1]).max() > 0 and np.all(got["dx"][cnt == 0] == 0)
    if row["geom"]:
        tk, tm = R.geom_bounds(d["x"], dwf, q, s, inds, dk, md, EXTENT, row["influence"], row["aggregation"], dmin)
        _check(got["d_dkp"], rdk, tk, "d deformed_kp")
        if md is not None:
            _check(got["d_mod"], rdm, tm, "d modulations")


def _run_with_points(row, d, gpu, Q, S, dwf, dmin):
    """_run on given point tensors (the ones a scheduling order was registered for)"""
    from weasal_amd import ops
    inds = torch.from_numpy(d["inds"]).to(gpu)
    X = _gpu_x(d["x"], row["dtype"], row["view"], gpu)
    _check_plan_on_device(row, X, Q, S, dwf, gpu)
    if dwf is not None:
        X = X.detach().requires_grad_(True)
    wf, _ = ops.kpconv_gather(X, Q, S, inds, torch.from_numpy(d["kp"]).to(gpu), EXTENT, row["influence"], row["aggregation"])
    out = dict(wf=wf.detach().float().cpu().numpy(), min_d2=None)
    if dwf is not None:
        wf.backward(torch.from_numpy(dwf).to(gpu).to(wf.dtype))
        out["dx"] = X.grad.float().cpu().numpy()
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------------------------
# K4G
# ------------------------------------------------------------------------------------------------------------------
_BATCHES = {}


def _slab_batch(gpu):
    if "slab" not in _BATCHES:
        from weasal_amd import config as wcfg, pyramid, synthetic
        cfg = wcfg.DALESPLConfig()
        pts, feats, labels, lens = synthetic.make_inputs(11, 1, 8000, 10.0, cfg.in_features_dim)
        pts, feats, labels = (torch.from_numpy(a).to(gpu) for a in (pts, feats, labels))
        _BATCHES["slab"] = (cfg, pyramid.build_batch(cfg, pts, feats, labels, lens, GRID_SLAB_LIMITS))
    return _BATCHES["slab"]


def _wide_batch(gpu):
    if "wide" not in _BATCHES:
        from weasal_amd import config as wcfg, pyramid
        from conftest import sphere
        cfg = wcfg.DALESDeformF32Config()
        pts = sphere(np.random.default_rng(5), 7000, 5.2)
        np.random.seed(2)
        batch = pyramid.build_batch(cfg, torch.from_numpy(pts).to(gpu), torch.ones((7000, 3), device=gpu),
                                    torch.zeros(7000, dtype=torch.int64, device=gpu), np.array([7000], np.int32),
                                    GRID_WIDE_LIMITS)
        _BATCHES["wide"] = (cfg, batch)
    return _BATCHES["wide"]


def _grid_dx(p, inds, dwf, kp, extent, kw, use_grid, x_dtype):
    from weasal_amd import ops
    ops.GRID_BACKWARD = use_grid
    x = torch.zeros(p.shape[0], dwf.shape[2], device=p.device, dtype=x_dtype, requires_grad=True)
    wf, _ = ops.kpconv_gather(x, p, p, inds, kp, extent, **kw)
    wf.backward(dwf)
    return x.grad.float()


def _grid_case(gpu, batch, cfg, lvl, ci, variant, bf, wide):
    """(grid-walk dx, index-order dx, table dx, per-element bound of |grid-walk - table|)"""
    from weasal_amd import _lib, ops
    sorted_switch = C.c_int.in_dll(_lib.lib(), "ws_kpconv_grid_sorted")
    p, inds = batch.points[lvl], batch.neighbors[lvl]
    grid = ops._grid_for(inds)
    assert grid is not None and grid.ns == p.shape[0]
    assert (grid.max_count > ops.GRID_NARROW_MAX) == wide, (grid.max_count, wide)
    r = cfg.first_subsampling_dl * cfg.conv_radius * 2 ** lvl
    extent = r * cfg.KP_extent / cfg.conv_radius
    gen = torch.Generator(device=gpu).manual_seed(ci * 7 + lvl)
    kp = torch.randn(15, 3, device=gpu, generator=gen) * (0.6 * r)
    kw = {}
    if variant == "deformable":
        kw = dict(deformed_kp=kp[None] + 0.1 * r * torch.randn(p.shape[0], 15, 3, device=gpu, generator=gen),
                  modulations=torch.rand(p.shape[0], 15, device=gpu, generator=gen), want_min_d2=True)
    elif variant == "gaussian-closest":
        kw = dict(influence="gaussian", aggregation="closest")
    dt = torch.bfloat16 if bf else torch.float32
    dwf = torch.randn(p.shape[0], 15, ci, device=gpu, generator=gen).to(dt)
    ordered = ops._order_for(p) is not None
    dx_like = torch.empty(p.shape[0], ci, device=gpu, dtype=dt)

    def asked(sort):
        kernel, args, keys = report("bwd_x_grid_wide" if wide else "bwd_x_grid", p.shape[0], p.shape[0], ci, dwf.data_ptr(),
                                    dx_like.data_ptr(), dtype="bf16" if bf else "f32", deformed=variant == "deformable",
                                    modulated=variant == "deformable", influence=kw.get("influence", "linear"),
                                    aggregation=kw.get("aggregation", "sum"), ordered=ordered)
        want = grid_plan(ci, variant, "bf16" if bf else "f32", wide, sort, ordered)
        assert (kernel, args, keys["ilv"]) == (want[0], table_launch(*want[:2])[1], want[2]), (kernel, args, keys)
    try:
        sorted_switch.value = 1
        asked(True)
        idx_order = _grid_dx(p, inds, dwf, kp, extent, kw, True, dt)
        sorted_switch.value = 0
        asked(False)
        walk = _grid_dx(p, inds, dwf, kp, extent, kw, True, dt)
        table = _grid_dx(p, inds, dwf, kp, extent, kw, False, dt)
        mag = _grid_dx(p, inds, dwf.abs(), kp, extent, kw, False, dt)
        ckw = {k: v for k, v in kw.items() if k not in ("influence", "aggregation", "deformed_kp", "modulations", "want_min_d2")}
        mag1 = _grid_dx(p, inds, dwf.abs(), kp, extent, dict(ckw, influence="constant"), False, dt)
    finally:
        sorted_switch.value = 0
        ops.GRID_BACKWARD = True
    assert int(grid.overflow.item()) == 0
    ns = p.shape[0]
    flat = inds.reshape(-1)
    n = 15.0 * torch.bincount(flat[flat < ns], minlength=ns)[:ns].double() + 6.0
    tmax = 0.0
    if variant == "gaussian-closest":       # largest |t| = d2 / (2 sigma^2) over the real (pair, kernel point) triples
        real = inds < ns
        nb = (p.double()[inds.clamp(max=ns - 1)] - p.double()[:, None, :])[real]
        d2 = ((nb[:, None, :] - kp.double()[None]) ** 2).sum(-1)
        tmax = float(d2.max()) / (2 * (float(np.float32(extent)) * 0.3) ** 2)
    c1, c2 = R.weight_constants("gaussian" if variant == "gaussian-closest" else "linear", tmax)
    tol = 2 * (n[:, None] + c1) * R.U * mag.double() + 2 * c2 * R.U * mag1.double()
    if bf:
        tol = tol + 2.0 ** -7 * table.abs().double()       # each side rounded to bf16 once
    return walk, idx_order, table, tol


@pytest.mark.parametrize("ci,variant,rows", GRID_SLAB, ids=["ci%d-%s-%s" % cv for cv in GRID_SLAB])
def test_grid_backward_slab_vs_table(gpu, ci, variant, rows):
    """K4G slab form (kpconv_gather_bwd_x_grid_kernel<15, G, MODE, VEC, T, SORT>) on levels 0-2 of a truncated pyramid:
    bit-identical to the table form in index order, within the per-element bound in grid-walk order"""
    cfg, batch = _slab_batch(gpu)
    batch.activate()
    for lvl in range(3):
        walk, idx_order, table, tol = _grid_case(gpu, batch, cfg, lvl, ci, variant, rows == "bf16", False)
        assert torch.equal(idx_order, table), (lvl, float((idx_order - table).abs().max()))
        msg = R.describe(walk.cpu().numpy(), table.cpu().numpy(), tol.cpu().numpy(), "dx level %d" % lvl)
        assert not msg, msg


@pytest.mark.parametrize("ci,rows", GRID_WIDE, ids=["ci%d-%s" % cv for cv in GRID_WIDE])
def test_grid_backward_wide_vs_table(gpu, ci, rows):
    """K4G wide form (kpconv_gather_bwd_x_gridw_kernel<15, G, 0, VEC, NCH, T>) on rows of several hundred neighbours
    (the config-5 limits): within the per-element bound of the table form (summed in walk order either way)"""
    cfg, batch = _wide_batch(gpu)
    batch.activate()
    walk, idx_order, table, tol = _grid_case(gpu, batch, cfg, 0, ci, "rigid", rows == "bf16", True)
    msg = R.describe(walk.cpu().numpy(), table.cpu().numpy(), tol.cpu().numpy(), "dx")
    assert not msg, msg
