"""CPU: the kernel sizes of the KPConv gather entries, asked of the library without a device.

ws_kpconv_gather_variant_k formats the plan the launchers follow for k kernel points (kpconv.hip); pointers are stand-in
addresses, nothing is read or launched.
* k = 15 answers exactly what ws_kpconv_gather_variant answers, for every row of the K = 15 branch table
  (tests/test_kpconv_branches_gpu.py: BRANCHES) and for the table-free backward cases.
* k in {9, 13}: the same kernel with the size in its text -- K=<k> where the kernel has a K argument, a leading "K=<k>, " in
  the matrix-core forward's list -- for every f32 row; and for every row of the K = 9 / 13 table of
  tests/test_kpconv_ksize_gpu.py, which states its launches independently.
* k in {7, 11, 16, 20}, bf16 rows with k = 13 and the deformable fast path (MODE 2) with k = 13 are refused with
  WS_ERR_UNSUPPORTED and a message that lists the built sizes; ws_kpconv_supported_k agrees with all of it.
"""
import ctypes as C

import pytest

import test_kpconv_branches_gpu as GB
import test_kpconv_ksize_gpu as KS
from weasal_amd import _lib, ops

UNSUPPORTED = 2
BUILT = (9, 13, 15)


def last_error():
    msg = _lib.lib().ws_last_error()
    return msg.decode() if msg else ""


def ask(op, k, nq, ns, ci, a, b, dtype="f32", deformed=False, modulated=False, influence="linear", aggregation="sum",
        rows_sorted=False, ordered=False):
    """(rc, text) of ws_kpconv_gather_variant_k, or of ws_kpconv_gather_variant when k is None"""
    lib = _lib.lib()
    buf = C.create_string_buffer(256)
    head = (GB.GATHER_OPS[op], nq, ns, ci, a, b, int(deformed), int(modulated), ops.INFLUENCE[influence], ops.AGGREGATION[aggregation],
            int(dtype == "bf16"), int(rows_sorted), int(ordered))
    rc = lib.ws_kpconv_gather_variant(*head, buf, 256) if k is None else lib.ws_kpconv_gather_variant_k(*head, k, buf, 256)
    return rc, buf.value.decode()


def row_questions(row):
    """the reporter questions of a branch-table row: (op, kwargs) for its forward, K4 and K6 launches"""
    off = 1 if row["view"] == "offset" else 0
    es = 2 if row["dtype"] == "bf16" else 4
    p = lambda name: GB.fake_ptr(name, off if name == "x" else 0, es)
    nq = row["nq"]
    ns = {"self": nq, "distinct": nq + 37, "hub": 2001, "dense": 2400}[row["queries"]]
    kw = dict(dtype=row["dtype"], deformed=row["deform"] is not None, modulated=row["deform"] == "defmod",
              influence=row["influence"], aggregation=row["aggregation"], ordered=row["order"])
    out = [("fwd", dict(kw, nq=nq, ns=ns, ci=row["ci"], a=p("x"), b=p("wf"), rows_sorted=row["rows_sorted"]))]
    if row["bwd"]:
        out.append(("bwd_x", dict(kw, nq=nq, ns=ns, ci=row["ci"], a=p("dwf"), b=p("dx"))))
    if row["geom"]:
        out.append(("bwd_geom", dict(kw, nq=nq, ns=ns, ci=row["ci"], a=p("x"), b=p("dwf"))))
    return out


def sized(text, k):
    """the K = 15 text with the size k in it, as the header describes"""
    if text.startswith(GB.MF + "<"):
        return text.replace(GB.MF + "<", GB.MF + "<K=%d, " % k, 1)
    assert "<K=15, " in text, text
    return text.replace("<K=15, ", "<K=%d, " % k, 1)


@pytest.mark.parametrize("row", GB.BRANCHES, ids=[r["id"] for r in GB.BRANCHES])
def test_k15_is_byte_identical_and_other_sizes_carry_the_size(row):
    for op, kw in row_questions(row):
        rc0, base = ask(op, None, **kw)
        assert rc0 == 0, last_error()
        assert ask(op, 15, **kw) == (0, base)
        for k in (9, 13):
            rc, text = ask(op, k, **kw)
            if row["dtype"] == "bf16":
                assert rc == UNSUPPORTED and "K=9, K=13 and K=15" in last_error() and "bf16" in last_error()
            else:
                assert (rc, text) == (0, sized(base, k)), (row["id"], op, k, text)


def test_k15_grid_reporters_unchanged_and_sized():
    for op in ("bwd_x_grid", "bwd_x_grid_wide"):
        for ci in (3, 4, 32, 64, 128, 256):
            for ordered in (False, True):
                kw = dict(nq=5000, ns=5000, ci=ci, a=GB.fake_ptr("dwf"), b=GB.fake_ptr("dx"), ordered=ordered)
                rc0, base = ask(op, None, **kw)
                assert rc0 == 0 and ask(op, 15, **kw) == (0, base)
                for k in (9, 13):
                    assert ask(op, k, **kw) == (0, sized(base, k))


@pytest.mark.parametrize("row", KS.BRANCHES, ids=[r["id"] for r in KS.BRANCHES])
def test_ksize_table_names_what_the_library_launches(row):
    """every row of the K = 9 / 13 table, with stand-in addresses of the alignment the GPU run has"""
    nq = row["nq"]
    ns = KS.supports_of(row)
    ptr = lambda name: GB.fake_ptr(name)
    assert KS.check_row_plan(row, ptr, nq, ns) == 1 + (row["bwd"] is not None) + (row["geom"] is not None)


def test_ksize_table_covers_both_sizes_alike():
    by_k = {k: sorted(r["id"].split("_", 1)[1] for r in KS.BRANCHES if r["k"] == k) for k in (9, 13)}
    assert by_k[9] == by_k[13] and len(by_k[9]) >= 30


@pytest.mark.parametrize("k", [7, 11, 16, 20])
def test_unbuilt_sizes_are_refused(k):
    lib = _lib.lib()
    for mode in (0, 1, 2):
        for bf in (0, 1):
            assert lib.ws_kpconv_supported_k(k, bf, mode) == 0
    for op in GB.GATHER_OPS:
        rc, _ = ask(op, k, 600, 600, 32, GB.fake_ptr("x"), GB.fake_ptr("wf"), deformed=op.endswith("_def"))
        assert rc == UNSUPPORTED, op
        msg = last_error()
        assert "num_kernel_points=%d" % k in msg and "K=9, K=13 and K=15" in msg, msg


def test_bf16_rows_and_mode2_are_15_only():
    lib = _lib.lib()
    for k in BUILT:
        for mode in (0, 1, 2):
            for bf in (0, 1):
                want = 1 if (k == 15 or (not bf and mode != 2)) else 0
                assert lib.ws_kpconv_supported_k(k, bf, mode) == want, (k, bf, mode)
    assert lib.ws_kpconv_supported_k(15, 0, 3) == 0 and lib.ws_kpconv_supported_k(15, 0, -1) == 0
    a, b = GB.fake_ptr("x"), GB.fake_ptr("wf")
    # bf16 rows, k = 13: every generic entry
    for op in ("fwd", "bwd_x", "bwd_geom", "bwd_x_grid"):
        rc, _ = ask(op, 13, 600, 600, 32, a, b, dtype="bf16")
        assert rc == UNSUPPORTED and "num_kernel_points=13" in last_error() and "K=9, K=13 and K=15" in last_error(), op
        assert ask(op, 15, 600, 600, 32, a, b, dtype="bf16")[0] == 0
    # MODE 2, k = 13: the four entries of the deformable fast path (the wide grid form with packed kernel points)
    for op, kw in (("fwd_def", {}), ("bwd_x_def", {}), ("bwd_geom_def", {}), ("bwd_x_grid_wide", dict(deformed=True))):
        rc, _ = ask(op, 13, 600, 600, 32, a, b, **kw)
        assert rc == UNSUPPORTED and "num_kernel_points=13" in last_error() and "K=9, K=13 and K=15" in last_error(), op
        assert ask(op, 15, 600, 600, 32, a, b, **kw)[0] == 0
    # ... while the rigid wide grid form runs the new sizes
    assert ask("bwd_x_grid_wide", 13, 600, 600, 32, a, b)[0] == 0


def test_python_guards_ask_the_library():
    import torch
    assert ops.kernel_size_supported(9) and ops.kernel_size_supported(13, mode=1) and ops.kernel_size_supported(15, True, 2)
    assert not ops.kernel_size_supported(13, bf16=True) and not ops.kernel_size_supported(9, mode=2) and not ops.kernel_size_supported(7)
    assert not ops.deform_fast_path_ok(torch.zeros(4, 32), 15, "linear", "sum")      # (a CPU tensor: never the fast path)
