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
* A sweep of the reporter over layer shapes lists the distinct plans in this module's scope (MODE 2 and FUSE belong to
  other modules); the tables reach every one of them.
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
