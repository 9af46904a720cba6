"""CPU side of tests/test_kpconv_branches_gpu.py: the per-element bound is not vacuous, and the branch table still names
what the dispatch launches.

* The bound helper (oracle/kpconv_branch_ref.py) passes the float32 oracle and flags a dropped neighbour, a zeroed
  kernel point of one channel, a partial last channel block shifted by one channel and a `closest` tie resolved to the
  later kernel point -- defects a per-tensor `max|a-b| <= tol * max|ref|` bound lets through where the values are small.
* The rows meant to straddle SPLIT_ROWS / SPLIT_NT (read from kpconv.hip) and ops.GRID_NARROW_MAX still do.
* Every row of BRANCHES, none excepted, agrees with the library's own statement of the launch: ws_kpconv_gather_variant,
  which formats the plan the launcher itself follows (kernel, every template argument, csplit; K4 and K6 where the row
  runs them), asked with stand-in addresses of the alignment the GPU run has (the view="offset" rows 4 bytes off).  The
  GRID_SLAB / GRID_WIDE cases are checked the same way (G, MODE, VEC, SORT or NCH, ilv with and without a point order).
* A sweep of the reporter over layer shapes lists the distinct plans of the generic entries and the rigid wide form (FUSE
  belongs to another module); the tables reach every one of them.
* The deformable fast path (DEF_BRANCHES and the queue-form MODE-2 cases of tests/test_kpconv_def_branches_gpu.py): every row
  asked of the reporter, the answers collected and compared with the list of instantiations the four deformable entries
  can launch; fwd_def swept over ci = 1..300 and bwd_geom_def over ci = 8..512 against the rules restated in Python.
* Self-tests of the float64 restatements the deformable tests use (oracle/kpconv_branch_ref.py, oracle/deform_ref.py):
  gradcheck at a tiny shape, analytic gradients against autograd, every bound finite and >= 0 and not vacuous.
* ws_kpconv_gather_fwd_variant (bench.py's roofline line) is the forward answer of that reporter for aligned rows at
  nq = SPLIT_ROWS, wherever the launcher accepts the layer.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import test_kpconv_branches_gpu as GB
from oracle import kpconv_branch_ref as R
from oracle.kpconv_ref import kpconv_gather_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(REPO, "weasal_amd", "csrc", "kpconv.hip")


def _hip_constant(name):
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, open(HIP).read())
    assert m, name
    return int(m.group(1))


# ------------------------------------------------------------------------------------------------------------------
# the bound is not vacuous
# ------------------------------------------------------------------------------------------------------------------
def _case(ci, ties=False, influence="linear", aggregation="sum", seed=0):
    rng = np.random.default_rng(seed)
    kp = GB._tie_kernel(rng) if ties else R.lattice_kernel(rng, 15, GB.KP_REACH)
    s = R.lattice_cloud(rng, 300, GB._half_for(300, 24))
    inds = R.brute_rows(s, s, GB.RADIUS, 40)
    assert R.extent_margin(s, s, inds, kp, GB.EXTENT) > 1e-6
    x = rng.standard_normal((300, ci)).astype(np.float32)
    ref, _ = R.ref_forward(x, s, s, inds, kp, GB.EXTENT, influence, aggregation)
    tol = R.fwd_bound(x, s, s, inds, kp, GB.EXTENT, influence, aggregation)
    return dict(kp=kp, s=s, inds=inds, x=x, ref=ref, tol=tol, influence=influence, aggregation=aggregation)


def _f32(c, x=None, inds=None, kp=None):
    """the float32 oracle: what a correct f32 kernel may return"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    wf, _ = kpconv_gather_ref(t(c["x"] if x is None else x), t(c["s"]), t(c["s"]), t(c["inds"] if inds is None else inds),
                              t(c["kp"] if kp is None else kp), float(np.float32(GB.EXTENT)), c["influence"], c["aggregation"])
    return wf.numpy()


def _flagged(c, got):
    return int(R.violations(got, c["ref"], c["tol"]).sum())


def test_bound_passes_the_float32_oracle():
    for c in (_case(20), _case(3, influence="gaussian"), _case(32, ties=True, influence="constant", aggregation="closest")):
        got = _f32(c)
        assert _flagged(c, got) == 0, R.describe(got, c["ref"], c["tol"], "f32 oracle")


def test_bound_flags_a_dropped_neighbour():
    c = _case(20)
    ns = c["s"].shape[0]
    # the real neighbour of row 5 with the smallest non-zero influence on any kernel point
    s_pad = np.concatenate([c["s"], np.full((1, 3), 1e6, np.float32)]).astype(np.float64)
    n = s_pad[c["inds"][5]] - c["s"][5].astype(np.float64)
    w = np.maximum(1 - np.sqrt(((n[:, None, :] - c["kp"][None].astype(np.float64)) ** 2).sum(-1)) / GB.EXTENT, 0).max(1)
    w[c["inds"][5] >= ns] = 0
    col = int(np.where(w > 0, w, np.inf).argmin())
    assert w[col] > 0
    inds = c["inds"].copy()
    inds[5, col] = ns
    got = _f32(c, inds=inds)
    assert _flagged(c, got) > 0


def test_bound_flags_a_zeroed_kernel_point_channel():
    c = _case(20)
    got = _f32(c)
    got[:, 7, 3] = 0.0
    assert _flagged(c, got) > 0


def test_bound_flags_a_shifted_partial_block():
    c = _case(20)          # blocks of 16 channels: the last block holds channels 16..19
    x = c["x"].copy()
    x[:, 16:19] = c["x"][:, 17:20]
    x[:, 19] = 0.0
    assert _flagged(c, _f32(c, x=x)) > 0


def test_bound_flags_a_tie_resolved_to_the_later_kernel_point():
    c = _case(32, ties=True, influence="constant", aggregation="closest")
    assert R.closest_tie_count(c["s"], c["s"], c["inds"], c["kp"]) > 0
    # the oracle on the reversed kernel points takes the LAST of the tied ones; reverse back
    got = _f32(c, kp=c["kp"][::-1].copy())[:, ::-1, :]
    assert _flagged(c, got) > 0


# ------------------------------------------------------------------------------------------------------------------
# the table straddles the constants
# ------------------------------------------------------------------------------------------------------------------
def _nt(table_args):
    return int(GB.table_launch(GB.MF, table_args)[1]["NT"])


def test_table_straddles_split_rows():
    split_rows, split_nt = _hip_constant("SPLIT_ROWS"), _hip_constant("SPLIT_NT")
    pairs = {}
    for r in GB.BRANCHES:
        if r["straddle"] and r["straddle"][0] == "SPLIT_ROWS":
            pairs.setdefault((r["straddle"][2], r["dtype"]), {})[r["straddle"][1]] = r
    assert {ci for ci, _ in pairs} >= {128, 256} and len(pairs) >= 4
    for (ci, dt), p in pairs.items():
        below, at = p["below"], p["at"]
        assert below["nq"] == split_rows - 1 and at["nq"] == split_rows, (ci, dt)
        assert below["ci"] == at["ci"] == ci
        # on both sides of the row count the dispatch switches: nt narrows to SPLIT_NT and the query splits into items
        assert _nt(at["targs"]) > split_nt and ci % split_nt == 0 and ci > 16 * split_nt, ci
        assert _nt(below["targs"]) == split_nt and below["csplit"] == -(-ci // (16 * split_nt)) > 1
        assert _nt(at["targs"]) == {128: 8, 256: 16}[ci] and at["csplit"] == 1


def test_table_straddles_grid_narrow_max():
    from weasal_amd import ops
    assert max(GB.GRID_SLAB_LIMITS) <= ops.GRID_NARROW_MAX < GB.GRID_WIDE_LIMITS[0]
    widths = {r["h"] for r in GB.BRANCHES if r["h"]}
    assert {1, 63, 64, 65, 129, 200} <= widths


# ------------------------------------------------------------------------------------------------------------------
# the tables agree with the library's own statement of each launch
# ------------------------------------------------------------------------------------------------------------------
def _ns(r):
    return {"self": r["nq"], "distinct": r["nq"] + 37, "hub": 2001, "dense": 2400}[r["queries"]]


def _row_ptr(r):
    off = 1 if r["view"] == "offset" else 0        # x = flat[1:]; wf, dwf and dx are fresh allocations
    return lambda name: GB.fake_ptr(name, off if name == "x" else 0, 2 if r["dtype"] == "bf16" else 4)


def test_table_matches_the_reporter():
    launches = 0
    for r in GB.BRANCHES:
        launches += GB.check_row_plan(r, _row_ptr(r), r["nq"], _ns(r))
        assert bool(r["geom"]) == (r["deform"] is not None and bool(r["bwd"])), r["id"]
        if r["dtype"] == "bf16":
            assert r["ci"] % 4 == 0 and r["view"] == "aligned", r["id"]
        if r["rows_sorted"]:
            assert r["entry"] == "ws_kpconv_gather_fwd_ex"
    assert launches == len(GB.BRANCHES) + sum(bool(r["bwd"]) + bool(r["geom"]) for r in GB.BRANCHES)


def _grid_report(ci, variant, dt, wide, ordered, ns=7000):
    return GB.report("bwd_x_grid_wide" if wide else "bwd_x_grid", ns, ns, ci, GB.fake_ptr("dwf"), GB.fake_ptr("dx"), dtype=dt,
                     deformed=variant == "deformable", modulated=variant == "deformable",
                     influence="gaussian" if variant == "gaussian-closest" else "linear",
                     aggregation="closest" if variant == "gaussian-closest" else "sum", ordered=ordered)


def test_grid_tables_match_the_reporter():
    from weasal_amd import _lib
    assert GB.GRID_ILV == _hip_constant("GRID_INTERLEAVE")
    switch = C.c_int.in_dll(_lib.lib(), "ws_kpconv_grid_sorted")
    cases = [(ci, v, dt, False) for ci, v, dt in GB.GRID_SLAB] + [(ci, "rigid", dt, True) for ci, dt in GB.GRID_WIDE]
    try:
        for sort in (False, True):
            switch.value = int(sort)
            for ci, variant, dt, wide in cases:
                for ordered in (False, True):
                    kernel, args, keys = _grid_report(ci, variant, dt, wide, ordered)
                    want = GB.grid_plan(ci, variant, dt, wide, sort, ordered)
                    assert (kernel, args, keys["ilv"]) == (want[0], GB.table_launch(*want[:2])[1], want[2]), (ci, variant, dt, wide)
                    # the interleaved assignment: 8 XCDs x min(ilv, 32-support chunks) workgroups
                    assert keys["grid"] == (8 * min(GB.GRID_ILV, -(-7000 // 32)) if ordered else 8 * -(-(-(-7000 // 4)) // 8))
    finally:
        switch.value = 0


def _plan_key(launch):
    kernel, args, keys = launch
    return (kernel,) + tuple(sorted(args.items())) + ((("vec4", keys["vec4"]),) if "vec4" in keys else ())


def test_tables_reach_every_plan_in_scope():
    """the reporter swept over layer shapes: every distinct (kernel, template arguments) it can name for the generic entries
    and the rigid wide form is one the tables run.  By family: matrix-core K3 5 NT x 2 row types x (MODE 0, MODE 0 + CUT,
    MODE 1, MODE 1 + DEF) = 40; pool K3 (G 1 / 4 for f32, G 1 for bf16) x (MODE 0, MODE 1, MODE 1 + DEF) = 9; K4 5 G x 2 MODE
    x (f32 VEC / scalar, bf16 VEC) = 30; K6 f32 vec4 0 / 1, bf16 vec4 1 = 3; K4G slab 30 x SORT = 60; K4G wide (G 1..8 with
    NCH 1, G 16 with NCH 1 / 2 / 4) x 3 = 21."""
    from weasal_amd import _lib
    split_rows = _hip_constant("SPLIT_ROWS")
    switch = C.c_int.in_dll(_lib.lib(), "ws_kpconv_grid_sorted")
    swept = set()
    try:
        for ci in list(range(1, 70)) + [96, 100, 128, 130, 192, 256, 260, 300]:
            for dt in ("f32", "bf16"):
                for off in (0, 1):
                    if dt == "bf16" and (ci % 4 or off):
                        continue                       # refused by every entry (module docstring of the GPU side)
                    es = 2 if dt == "bf16" else 4
                    x, wf, dwf, dx = GB.fake_ptr("x", off, es), GB.fake_ptr("wf"), GB.fake_ptr("dwf"), GB.fake_ptr("dx")
                    for influence, aggregation in (("linear", "sum"), ("gaussian", "sum"), ("constant", "closest")):
                        for deform in (None, "def", "defmod"):
                            kw = dict(dtype=dt, deformed=deform is not None, modulated=deform == "defmod", influence=influence,
                                      aggregation=aggregation)
                            for nq in (split_rows - 1, split_rows):
                                for srt in (False, True):
                                    swept.add(_plan_key(GB.report("fwd", nq, nq, ci, x, wf, rows_sorted=srt, **kw)))
                            swept.add(_plan_key(GB.report("bwd_x", 600, 600, ci, dwf, dx, **kw)))
                            if deform:
                                swept.add(_plan_key(GB.report("bwd_geom", 600, 600, ci, x, dwf, **kw)))
                            if not off:
                                for sort in (0, 1):
                                    switch.value = sort
                                    swept.add(_plan_key(GB.report("bwd_x_grid", 600, 600, ci, dwf, dx, **kw)))
                                switch.value = 0
                                if influence == "linear" and not deform:
                                    swept.add(_plan_key(GB.report("bwd_x_grid_wide", 600, 600, ci, dwf, dx, **kw)))
    finally:
        switch.value = 0
    reached = set()
    for r in GB.BRANCHES:
        reached.add(_plan_key(GB.table_launch(r["kernel"], r["targs"])))
        for key in ("bwd", "geom"):
            if r[key]:
                reached.add(_plan_key(GB.table_launch(*r[key])))
    for ci, variant, dt in GB.GRID_SLAB:
        for sort in (False, True):
            reached.add(_plan_key(GB.table_launch(*GB.grid_plan(ci, variant, dt, False, sort)[:2])))
    for ci, dt in GB.GRID_WIDE:
        reached.add(_plan_key(GB.table_launch(*GB.grid_plan(ci, "rigid", dt, True)[:2])))
    assert len(swept) == 40 + 9 + 30 + 3 + 60 + 21, len(swept)
    assert swept - reached == set(), sorted(swept - reached)
    assert reached - swept == set(), sorted(reached - swept)


def test_old_reporter_is_the_forward_plan_at_split_rows():
    """ws_kpconv_gather_fwd_variant = the forward answer of ws_kpconv_gather_variant for aligned rows at nq = SPLIT_ROWS"""
    from weasal_amd import _lib, ops
    lib = _lib.lib()
    split_rows = _hip_constant("SPLIT_ROWS")
    asked = 0
    for ci in range(1, 301):
        for mode in (0, 1, 2):
            for influence in ("linear", "constant", "gaussian"):
                for aggregation in ("sum", "closest"):
                    if mode == 2 and (influence, aggregation) != ("linear", "sum"):
                        continue
                    for dt in ("f32", "bf16"):
                        for srt in (0, 1):
                            new = C.create_string_buffer(256)
                            rc = lib.ws_kpconv_gather_variant(GB.GATHER_OPS["fwd_def" if mode == 2 else "fwd"], split_rows, split_rows, ci,
                                                              GB.fake_ptr("x"), GB.fake_ptr("wf"), int(mode == 1), 0,
                                                              ops.INFLUENCE[influence], ops.AGGREGATION[aggregation], int(dt == "bf16"), srt, 0,
                                                              new, 256)
                            old = C.create_string_buffer(256)
                            rc_old = lib.ws_kpconv_gather_fwd_variant(ci, mode, ops.INFLUENCE[influence], ops.AGGREGATION[aggregation],
                                                                      int(dt == "bf16"), srt, old, 256)
                            assert rc == rc_old, (ci, mode, dt)
                            if rc != 0:
                                assert dt == "bf16" and ci % 4, (ci, mode, dt)      # the launcher refuses the layer
                                continue
                            kernel, args, keys = GB.parse_launch(new.value.decode())
                            text = old.value.decode()
                            okernel, _, orest = text.partition("<")
                            oargs = [a.strip() for a in orest.partition(">")[0].split(",")]
                            oargs = dict(a.split("=") if "=" in a else ("T", a) for a in oargs)
                            assert oargs.pop("GS", "default") == "default"
                            assert (okernel, oargs) == (kernel, args), (text, new.value.decode())
                            assert keys["csplit"] == 1
                            assert text.endswith(" (sorted-row cutoff on)") == bool(keys.get("cut") and args["MODE"] == "0"), text
                            asked += 1
    assert asked > 300 * 2 * 14


# ------------------------------------------------------------------------------------------------------------------
# the deformable fast path (tests/test_kpconv_def_branches_gpu.py): table, reporter sweep, oracle self-tests
# ------------------------------------------------------------------------------------------------------------------
import test_kpconv_def_branches_gpu as DB      # noqa: E402
from oracle import deform_ref as DR           # noqa: E402


def _def_row_ptr(r):
    """x = flat[1:] on the offset rows, and dwf too on the f32 one; wf and dx are fresh allocations"""
    es = 2 if r["dtype"] == "bf16" else 4
    off = {"x": 1 if r["view"] == "offset" else 0, "dwf": 1 if (r["view"] == "offset" and r["dtype"] == "f32") else 0}
    return lambda name: GB.fake_ptr(name, off.get(name, 0), es)


def _tf(v):
    return "true" if v else "false"


# every instantiation the four deformable entries can launch.  Not in the list because no argument reaches them: the
# transposed-table and queue kernels with MODE 2, VEC = false on bf16 rows (rows_vec4_or_f32 refuses the rows), and the queue
# kernel with NCH > 1 below G = 16 (bwd_x_gridw_plan: NCH = 1 there).
DEF_INSTANTIATIONS = (
    [(GB.MF, dict(NT=str(nt), MODE="2", DEF="true", VECROW="true", T=t, CUT=_tf(cut)))
     for nt in (1, 2, 4, 8, 16) for t in ("float", "bf16") for cut in (False, True)] +
    [(GB.K4, dict(K="15", G=str(g), MODE="2", VEC=_tf(vec), T=t))
     for g in (1, 2, 4, 8, 16) for vec, t in ((True, "float"), (False, "float"), (True, "bf16"))] +
    [(GB.K4GW, dict(K="15", G=str(g), MODE="2", VEC=_tf(vec), NCH=str(nch), T=t))
     for g in (1, 2, 4, 8, 16) for vec, t in ((True, "float"), (False, "float"), (True, "bf16"))
     for nch in ((1, 2, 4) if g == 16 else (1,))] +
    [(DB.GD, dict(CK=str(ck), AREG=_tf(areg), T=t, CUT=_tf(cut)))
     for ck in (4, 8, 16, 32) for areg in (True, False) for t in ("float", "bf16") for cut in (False, True)])


def test_def_table_matches_the_reporter_and_reaches_every_instantiation():
    """every DEF_BRANCHES row and every queue-form MODE-2 case, asked with stand-in addresses; the set of answers is the set
    of instantiations the four deformable entries can launch"""
    ids = [r["id"] for r in DB.DEF_BRANCHES]
    assert len(set(ids)) == len(ids)
    reached = set()
    for r in DB.DEF_BRANCHES:
        ns = r["nq"] if r["queries"] == "self" else {"distinct": r["nq"] + 37, "hub": 2001, "dense": 2400}[r["queries"]]
        if r["cut"]:
            ns = 3200
        for srt in {r["rows_sorted"], False} if r["cut"] else {r["rows_sorted"]}:
            for launch in DB.check_def_plan(r, _def_row_ptr(r), r["nq"], ns, srt):
                reached.add(_plan_key(launch))
        # the row's own statement follows the rules of the plan functions
        nt = int(GB.table_launch(r["kernel"], r["targs"])[1]["NT"])
        if "fwd" not in r["refuse"]:
            assert nt == DB.fwd_nt(r["ci"], r["view"] == "aligned"), r["id"]
        assert (r["geom"] is None) or GB.table_launch(*r["geom"])[1]["CK"] == str(DB.geom_ck(r["ci"])[0]), r["id"]
        assert r["geom"] is not None or "geom" in r["refuse"] or r["ci"] % 16 == 0, r["id"]
        assert r["cut"] == r["rows_sorted"]
    for ci, dt in GB.GRID_WIDE:
        for ordered in (False, True):
            kernel, args, keys = GB.report("bwd_x_grid_wide", 7000, 7000, ci, GB.fake_ptr("dwf"), GB.fake_ptr("dx"), dtype=dt,
                                           deformed=True, modulated=True, ordered=ordered)
            want = DB.grid_def_plan(ci, dt, ordered)
            assert (kernel, args, keys["ilv"]) == (want[0], GB.table_launch(*want[:2])[1], want[2]), (ci, dt, ordered)
            reached.add(_plan_key((kernel, args, keys)))
    want = {_plan_key((k, a, {})) for k, a in DEF_INSTANTIATIONS}
    assert len(want) == 20 + 15 + 21 + 32
    assert want - reached == set(), sorted(want - reached)
    assert reached - want == set(), sorted(reached - want)
    widths = {r["h"] for r in DB.DEF_BRANCHES if r["queries"] == "dense"}
    assert widths == {1, 15, 16, 17, 63, 64, 65, 129, 200}


def test_def_reporter_sweep_follows_the_rules():
    """fwd_def over ci = 1..300 and bwd_geom_def over ci = 16..512 (and the widths between, refused), f32 and bf16, aligned and
    offset rows, sorted or not: NT, the even-ci rule for bf16, CK, AREG, CUT; bwd_x_def and the queue form: G, VEC, NCH"""
    from weasal_amd import _lib
    asked = 0
    for dt in ("f32", "bf16"):
        es, t = (2, "bf16") if dt == "bf16" else (4, "float")
        for srt in (False, True):
            for off in (0, 1):
                x, wf, dwf, dx = GB.fake_ptr("x", off, es), GB.fake_ptr("wf"), GB.fake_ptr("dwf", off, es), GB.fake_ptr("dx")
                kw = dict(dtype=dt, deformed=True, modulated=True, rows_sorted=srt)
                grid16 = GB.report("fwd_def", 600, 600, 16, wf, wf, **kw)[2]["grid"]
                for ci in range(1, 301):
                    nt = DB.fwd_nt(ci, not off)
                    if dt == "bf16" and nt == 1 and ci % 2:
                        with pytest.raises(_lib.WeasalHipError):
                            GB.report("fwd_def", 600, 600, ci, x, wf, **kw)
                    else:
                        kernel, args, keys = GB.report("fwd_def", 600, 600, ci, x, wf, **kw)
                        assert (kernel, args) == GB.table_launch(GB.MF, GB._mf(nt, 2, True, t, cut=srt))[:2], (ci, dt, off, srt)
                        assert keys["csplit"] == 1 and keys["grid"] == grid16, "the grid of the forward does not depend on ci"
                    vec = ci % 4 == 0 and not off
                    if dt == "bf16" and not vec:
                        with pytest.raises(_lib.WeasalHipError):
                            GB.report("bwd_x_def", 600, 600, ci, dwf, dx, **kw)
                        with pytest.raises(_lib.WeasalHipError):
                            GB.report("bwd_x_grid_wide", 600, 600, ci, dwf, dx, **kw)
                    else:
                        g = GB._k4g(ci)
                        kernel, args, _ = GB.report("bwd_x_def", 600, 600, ci, dwf, dx, **kw)
                        assert (kernel, args) == GB.table_launch(*GB._k4(g, 2, vec, t))[:2], (ci, dt, off)
                        kernel, args, _ = GB.report("bwd_x_grid_wide", 600, 600, ci, dwf, dx, **kw)
                        nch = 1 if (g < 16 or ci <= 64) else 2 if ci <= 128 else 4
                        assert kernel == GB.K4GW and args == dict(K="15", G=str(g), MODE="2", VEC=_tf(vec), NCH=str(nch), T=t), (ci, dt, off)
                    asked += 3
                for ci in range(8, 513, 8):
                    plan = DB.geom_ck(ci)
                    if plan is None or off:
                        with pytest.raises(_lib.WeasalHipError):
                            GB.report("bwd_geom_def", 600, 600, ci, x, wf, **kw)
                    else:
                        kernel, args, _ = GB.report("bwd_geom_def", 600, 600, ci, x, wf, **kw)
                        assert (kernel, args) == GB.table_launch(*DB._gd(plan[0], plan[1], t, srt))[:2], (ci, dt, srt)
                        assert plan[1] == (ci in (16, 32, 64, 128)) and ci % (4 * plan[0]) == 0
                        assert plan[1] or plan[0] == max(c for c in (4, 8, 16, 32) if ci % (4 * c) == 0)
                    asked += 1
    assert asked == 2 * 2 * 2 * (900 + 64)


def _tiny_case(seed=0, nq=6, ci=3):
    rng = np.random.default_rng(seed)
    kp = R.lattice_kernel(rng, 15, GB.KP_REACH)
    s = R.lattice_cloud(rng, 40, 0.4)
    q = s[:nq].copy()
    inds = R.brute_rows(q, s, GB.RADIUS, 9)
    inds[1] = s.shape[0]                                   # a row of shadow columns only
    dk = R.lattice_deformed(rng, kp, nq, 0.05)
    md = rng.uniform(0.25, 2.0, size=(nq, 15)).astype(np.float32)
    md[0, :3] = 0.0
    x = rng.standard_normal((40, ci)).astype(np.float32)
    return dict(q=q, s=s, inds=inds, kp=kp, dk=dk, md=md, x=x, rng=rng)


def test_branch_oracle_def_gradients_and_bounds():
    """the float64 reference of the deformable rows: its autograd gradients pass gradcheck at a tiny shape; every bound the
    deformable rows use is finite and >= 0; the shadow-row bound of min_d2 is the wider one"""
    c = _tiny_case()
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    ext = float(np.float32(GB.EXTENT))
    assert R.extent_margin(c["q"], c["s"], c["inds"], c["kp"], GB.EXTENT, c["dk"]) > 1e-6

    rows = torch.from_numpy(R.brute_rows(c["q"], c["s"], GB.RADIUS, 9))     # (no shadow-only row here: a finite difference on
                                                                            #  a squared distance of 3e12 resolves nothing)
    def f(x, dk, md):
        wf, mn = kpconv_gather_ref(x, t(c["q"]), t(c["s"]), rows, t(c["kp"]), ext, "linear", "sum", dk, md)
        return wf, mn
    # (kernel points moved off the lattice: two neighbours at exactly the same distance make the minimum non-differentiable)
    dk_off = c["dk"].astype(np.float64) + c["rng"].uniform(-1e-3, 1e-3, size=c["dk"].shape)
    assert torch.autograd.gradcheck(f, (t(c["x"]).requires_grad_(True), t(dk_off).requires_grad_(True), t(c["md"]).requires_grad_(True)),
                                    eps=1e-7, atol=1e-6)
    dwf = c["rng"].standard_normal((6, 15, 3)).astype(np.float32)
    dmin = c["rng"].standard_normal((6, 15)).astype(np.float32)
    ref, ref_min = R.ref_forward(c["x"], c["q"], c["s"], c["inds"], c["kp"], GB.EXTENT, "linear", "sum", c["dk"], c["md"])
    rdx, rdk, rdm = R.ref_backward(c["x"], dwf, c["q"], c["s"], c["inds"], c["kp"], GB.EXTENT, "linear", "sum", c["dk"], c["md"], dmin)
    assert np.all(ref[0, :3] == 0) and np.all(rdk[0, :3] == 2 * dmin[0, :3, None] * _argmin_offset(c)[0, :3]) and np.abs(rdm[0, :3]).max() > 0
    bounds = [R.fwd_bound(c["x"], c["q"], c["s"], c["inds"], c["kp"], GB.EXTENT, "linear", "sum", c["dk"], c["md"], 0.0, ref, True),
              R.dx_bound(dwf, c["q"], c["s"], c["inds"], c["kp"], GB.EXTENT, "linear", "sum", c["dk"], c["md"], 0.0, rdx, True, c["x"].shape),
              R.min_d2_bound(ref_min, c["q"], c["s"], c["inds"], c["dk"])]
    bounds += list(R.geom_bounds(c["x"], dwf, c["q"], c["s"], c["inds"], c["dk"], c["md"], GB.EXTENT, "linear", "sum", dmin))
    for b in bounds:
        assert np.all(np.isfinite(b)) and np.all(b >= 0)
    mb = bounds[2] / np.abs(ref_min)
    assert np.allclose(mb[1], 8 * R.U) and np.allclose(np.delete(mb, 1, 0), 4 * R.U)
    # the float32 oracle stays inside, a min_d2 taken from the wrong column does not
    assert R.worst_ratio(ref_min.astype(np.float32), ref_min, bounds[2])[0] <= 1.0
    wrong = ref_min.copy()
    wrong[2, 4] *= 1.0 + 2.0 ** -20
    assert R.violations(wrong, ref_min, bounds[2]).sum() == 1
    assert R.worst_ratio(np.ones(3), np.ones(3), np.zeros(3)) == (0.0, 3) and R.worst_ratio(np.ones(1), np.zeros(1), 0.0)[0] == np.inf
    # cutoff_counts on rows it can judge by hand: one query at the origin, its row along a ray, all kernel points at one place
    zero = np.zeros((1, 3), np.float32)
    s = np.zeros((70, 3), np.float32)
    s[:, 0] = (np.arange(70) + 1) * R.STEP
    kq = np.full((1, 15, 3), R.KP_SHIFT, np.float32)
    kq[0, :, 0] += 69 * R.STEP                        # at the far end: its nearest column is the last, the reach covers the row
    assert R.cutoff_counts(zero, s, np.arange(70)[None], kq, GB.EXTENT) == (1, 15, 0, 0, 0)
    near = np.full((1, 15, 3), R.KP_SHIFT, np.float32)  # at the query, and a row that starts 41 steps out: beyond the reach
    assert R.cutoff_counts(zero, s[40:], np.arange(30)[None], near, GB.EXTENT) == (0, 0, 1, 0, 0)
    ray = np.zeros((200, 3))
    ray[:, 0] = (np.arange(200) + 1) * 0.01
    kq = np.zeros((1, 15, 3))
    kq[0, :, 0] = 0.9                                 # reach 0.9 + 0.3 (the first chunk ends at 0.64: 0.26 + 0.9 is less): 120 columns
    assert R.cutoff_counts(zero, ray, np.arange(200)[None], kq, GB.EXTENT)[3:] == (1, 0)
    kq[0, :, 0] = 1.2                                 # what could lower a minimum reaches farther: 0.56 + 1.2, 176 columns
    assert R.cutoff_counts(zero, ray, np.arange(200)[None], kq, GB.EXTENT)[3:] == (0, 1)
    kq[0, :, 0] = 1.7                                 # 1.06 + 1.7: the whole row is walked
    assert R.cutoff_counts(zero, ray, np.arange(200)[None], kq, GB.EXTENT)[3:] == (0, 0)


def _argmin_offset(c):
    """kp - n at the arg-min column of every (query, kernel point), float64"""
    s_pad = np.concatenate([c["s"].astype(np.float64), np.full((1, 3), 1e6)])
    n = s_pad[c["inds"]] - c["q"][:, None, :].astype(np.float64)
    sq = ((n[:, :, None, :] - c["dk"][:, None].astype(np.float64)) ** 2).sum(-1)
    arg = sq.argmin(1)
    nstar = np.take_along_axis(n[:, :, None, :].repeat(15, 2), arg[:, None, :, None], 1)[:, 0]
    return c["dk"].astype(np.float64) - nstar


def test_deform_oracle_gradients_and_bounds():
    """oracle/deform_ref.py: the analytic gradients agree with float64 autograd of the torch restatements (which pass
    gradcheck); every bound is finite and >= 0; the float32 evaluation of the same formulas stays inside"""
    rng = np.random.default_rng(1)
    kp = (rng.standard_normal((15, 3)) * 0.3).astype(np.float32)
    ext = float(np.float32(1.2))
    for modulated in (False, True):
        off = rng.standard_normal((4, 60 if modulated else 45)).astype(np.float32)
        O = torch.from_numpy(off.astype(np.float64)).requires_grad_(True)
        KP = torch.from_numpy(kp.astype(np.float64))
        assert torch.autograd.gradcheck(lambda o: DR.prepare_torch(o, KP, ext, modulated), (O,))
        ref, tol = DR.prepare_ref(off, kp, 1.2, modulated)
        out = DR.prepare_torch(O, KP, ext, modulated)
        assert np.allclose(out.detach().numpy(), ref, rtol=1e-14, atol=0)
        d4 = rng.standard_normal((4, 15, 4))
        d3 = rng.standard_normal((4, 15, 3))
        for second in (None, d3):
            O.grad = None
            loss = (out * torch.from_numpy(d4)).sum() + ((out[..., :3] * torch.from_numpy(second)).sum() if second is not None else 0)
            loss.backward(retain_graph=True)
            g, gt = DR.prepare_bwd_ref(off, d4, second, 1.2, modulated, tol[..., 3])
            assert np.allclose(O.grad.numpy(), g, rtol=1e-12, atol=1e-15)
            assert np.all(np.isfinite(gt)) and np.all(gt >= 0) and np.all(np.isfinite(tol)) and np.all(tol >= 0)
        f32 = DR.prepare_torch(torch.from_numpy(off), torch.from_numpy(kp), np.float32(1.2), modulated).numpy()
        assert R.violations(f32[..., :3], ref[..., :3], tol[..., :3]).sum() == 0
        assert R.violations(f32[..., 3], ref[..., 3], tol[..., 3] + 2 * R.U * np.abs(ref[..., 3])).sum() == 0     # (torch's own sigmoid)
    dkp = (rng.standard_normal((5, 15, 3)) * 1.1).astype(np.float32)
    md = rng.standard_normal((5, 15)).astype(np.float32)
    assert DR.repulse_margins(dkp, 1.2, 1.2).min() > 1e-5
    Dk = torch.from_numpy(dkp.astype(np.float64)).requires_grad_(True)
    Md = torch.from_numpy(md.astype(np.float64)).requires_grad_(True)
    # (the other points are detached: the derivative autograd returns is that of the function with them held fixed)
    fixed = Dk.detach().clone()
    assert torch.autograd.gradcheck(lambda a, b: DR.regularizer_torch(a, b, ext, ext, others=fixed), (Dk, Md), eps=1e-7, atol=1e-7)
    out = DR.regularizer_torch(Dk, Md, ext, ext)
    ref, tol = DR.regularizer_ref(dkp, md, 1.2, 1.2)
    assert np.allclose(out.detach().numpy(), ref, rtol=1e-13) and np.all(tol > 0) and np.all(np.isfinite(tol))
    g = np.array([0.7, -1.3])
    out.backward(torch.from_numpy(g))
    rk, tk, rm, tm = DR.regularizer_bwd_ref(dkp, md, 1.2, 1.2, g)
    assert np.allclose(Dk.grad.numpy(), rk, rtol=1e-11, atol=1e-15) and np.allclose(Md.grad.numpy(), rm, rtol=1e-13)
    for b in (tk, tm):
        assert np.all(np.isfinite(b)) and np.all(b >= 0)
    out32 = DR.regularizer_torch(torch.from_numpy(dkp), torch.from_numpy(md), np.float32(1.2), np.float32(1.2)).numpy()
    assert R.violations(out32, ref, tol).sum() == 0
    # a dropped pair term or a sign error in the gradient is outside the bound
    assert R.violations(rk * np.array([1, 1, -1.0]), rk, tk).sum() > 0
    assert R.violations(ref * (1 + 2.0 ** -17), ref, tol).sum() == 2
