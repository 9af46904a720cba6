"""CPU side of tests/test_kpconv_branches_gpu.py: the per-element bound is not vacuous, and the branch table still names
what the dispatch launches.

* The bound helper (oracle/kpconv_branch_ref.py) passes the float32 oracle and flags a dropped neighbour, a zeroed
  kernel point of one channel, a partial last channel block shifted by one channel and a `closest` tie resolved to the
  later kernel point -- defects a per-tensor `max|a-b| <= tol * max|ref|` bound lets through where the values are small.
* The rows meant to straddle SPLIT_ROWS / SPLIT_NT (read from kpconv.hip) and ops.GRID_NARROW_MAX still do.
* Every row's kernel and template arguments agree with a restatement of the dispatch (gather_fwd_impl,
  gather_bwd_x_impl, gather_bwd_geom_impl), and, where it applies, with the library's own name for the forward kernel:
  ws_kpconv_gather_fwd_variant (bench.py's roofline line).  That reporter takes neither nq nor the row alignment, so it
  does not describe the SPLIT_NT narrowing / csplit items (rigid linear / sum below SPLIT_ROWS queries) or the NT = 1
  fallback of unaligned rows: it is asked only about aligned rows outside those branches.
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
def _nt(ci):
    return 1 if ci <= 16 else 2 if ci <= 32 else 4 if ci <= 64 else 8 if ci <= 128 else 16


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
        assert _nt(ci) > split_nt and ci % split_nt == 0 and ci > 16 * split_nt, ci
        assert "NT=%d," % split_nt in below["targs"] and below["csplit"] == -(-ci // (16 * split_nt)) > 1
        assert "NT=%d," % _nt(ci) in at["targs"] and at["csplit"] == 1


def test_table_straddles_grid_narrow_max():
    from weasal_amd import ops
    assert max(GB.GRID_SLAB_LIMITS) <= ops.GRID_NARROW_MAX < GB.GRID_WIDE_LIMITS[0]
    widths = {r["h"] for r in GB.BRANCHES if r["h"]}
    assert {1, 63, 64, 65, 129, 200} <= widths


# ------------------------------------------------------------------------------------------------------------------
# the table agrees with the dispatch and with the library's own name
# ------------------------------------------------------------------------------------------------------------------
def _fwd_dispatch(r, split_rows, split_nt):
    """(kernel, template args, csplit) as gather_fwd_impl picks them"""
    ci, bf = r["ci"], r["dtype"] == "bf16"
    t = "bf16" if bf else "float"
    aligned = r["view"] == "aligned"
    deff = r["deform"] is not None
    fast = r["influence"] == "linear" and r["aggregation"] == "sum"
    if ci > 4:
        fastm = fast and not deff
        nt = _nt(ci)
        vecrow = ci % nt == 0 and (nt == 1 or aligned)
        if not vecrow:
            nt = 1
        if fastm and not r["rows_sorted"] and r["nq"] < split_rows and nt > split_nt and ci % split_nt == 0:
            nt = split_nt
        csplit = 1
        if fastm and not r["rows_sorted"] and r["nq"] < split_rows and ci > 16 * nt:
            csplit = -(-ci // (16 * nt))
        mode = 0 if fastm else 1
        return GB.MF, GB._mf(nt, mode, deff, t, cut=fastm and r["rows_sorted"]), csplit
    vec4 = ci % 4 == 0 and aligned
    mode = 0 if (fast and not deff) else 1
    return GB.VF, GB._vf(1 if vec4 else 4, mode, deff, vec4, 4 if vec4 else 1, t), 1


def test_table_matches_the_dispatch():
    split_rows, split_nt = _hip_constant("SPLIT_ROWS"), _hip_constant("SPLIT_NT")
    for r in GB.BRANCHES:
        assert (r["kernel"], r["targs"], r["csplit"]) == _fwd_dispatch(r, split_rows, split_nt), r["id"]
        t = "bf16" if r["dtype"] == "bf16" else "float"
        fast = r["influence"] == "linear" and r["aggregation"] == "sum" and r["deform"] is None
        if r["bwd"]:
            assert r["bwd"] == GB._k4(GB._k4g(r["ci"]), 0 if fast else 1, r["ci"] % 4 == 0, t), r["id"]
        if r["geom"]:
            assert r["geom"] == GB._k6(t, r["ci"] % 4 == 0), r["id"]
        assert bool(r["geom"]) == (r["deform"] is not None and bool(r["bwd"])), r["id"]
        if r["dtype"] == "bf16":
            assert r["ci"] % 4 == 0 and r["view"] == "aligned", r["id"]
        if r["rows_sorted"]:
            assert r["entry"] == "ws_kpconv_gather_fwd_ex"


def _parse(name):
    m = re.match(r"(\w+)<(.*)>", name.split(" (")[0])
    assert m, name
    args = {}
    for a in m.group(2).split(","):
        a = a.strip()
        k, _, v = a.partition("=")
        if not _:
            k, v = "T", a
        args[k.strip()] = v.strip()
    args.pop("GS", None)
    return m.group(1), args


def test_table_matches_the_variant_reporter():
    from weasal_amd import _lib, ops
    lib = _lib.lib()
    split_rows = _hip_constant("SPLIT_ROWS")
    asked = 0
    for r in GB.BRANCHES:
        fastm = r["influence"] == "linear" and r["aggregation"] == "sum" and r["deform"] is None
        if r["view"] != "aligned" or (r["ci"] > 4 and fastm and not r["rows_sorted"] and r["nq"] < split_rows):
            continue           # the reporter knows neither the alignment nor nq (module docstring)
        buf = C.create_string_buffer(256)
        _lib.check(lib.ws_kpconv_gather_fwd_variant(r["ci"], 1 if r["deform"] else 0, ops.INFLUENCE[r["influence"]],
                                                    ops.AGGREGATION[r["aggregation"]], 1 if r["dtype"] == "bf16" else 0,
                                                    1 if r["rows_sorted"] else 0, buf, 256))
        kernel, args = _parse(buf.value.decode())
        want_kernel, want = _parse("%s<%s>" % (r["kernel"], r["targs"]))
        assert kernel == want_kernel and args == want, (r["id"], buf.value.decode())
        asked += 1
    assert asked >= 30
