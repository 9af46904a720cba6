"""Every branch of grid subsampling (weasal_amd/csrc/subsample.hip) against the map walk of the port oracle
(oracle/ws_oracle.cpp through oracle/geom.py: a real std::unordered_map per element, the reference's arithmetic).  Row order,
cell keys, counts, barycentres, feature means and labels are bit-exact: every comparison here is np.array_equal.

The data sets and case tables live in oracle/subsample_ref.py; tests/test_subsample_branches_cpu.py asserts that they hold
what the cases rely on (exact cell counts, the key 2^64 - 1, distinct labels per cell, ties), holds the port to the compiled
reference where that is defined, and shows that the comparison used here rejects small mutations.

  row counts     cell counts either side of every rehash the order kernel replays (13|14 ... 2357|2358) and of the second
                 chunk of its block scan (1024|1025), alone and in one batch with empty elements first, twice in a row, last
  rounding       points on and one ulp either side of k dl, near 4e5, negative, and with the origin above the minimum
  wrapped_key    a cell whose key is 2^64 - 1, the hash table's empty marker
  emission       fd 1/3/5, ld 1-D/1/2/3, max_p 0/7/m/m+1, reference and first-seen order
  labels         histograms of 13|14, 29|30, 48 and of 49, 60, 130 distinct labels, maxima tied and unique
  crowded        4096 points in one cell: list sort, long sequential sums, hash contention
  scan           n = 1, 4095, 4096, 4097, 8193 (the tile of ws_exclusive_scan_i32); elements of 32|33 points (64|128 slots)
  workspace      large then small then features + labels on one workspace; fill after a failed plan
  rotation       64 elements (kernel-argument table) and 65 (device lengths)
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import geom
from oracle import subsample_ref as S
from weasal_amd import _lib, ops
from weasal_amd._lib import current_stream, ptr

pytestmark = pytest.mark.gpu

_PORT = {}


def dev(a, gpu):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(gpu)      # (a copy: the sets are read-only)


def port(d, max_p=0):
    """dict(p, lens, keys, counts[, f][, c]) of the port oracle; computed once per (data, max_p) and never changed"""
    key = (id(d), max_p)
    if key not in _PORT:
        r = geom.subsample_batch(d["p"], d["lens"], features=d["f"], classes=d["c"], sampleDl=d["dl"], max_p=max_p,
                                 with_keys=True)
        out = dict(p=r[0], lens=r[1], keys=r[-2], counts=r[-1])
        rest = list(r[2:-2])
        if d["f"] is not None:
            out["f"] = rest.pop(0)
        if d["c"] is not None:
            out["c"] = rest.pop(0)
        for a in out.values():
            a.setflags(write=False)
        _PORT[key] = (d, out)                                          # (keeps d alive: its id stays its own)
    return _PORT[key][1]


def run(gpu, d, max_p=0, reference_order=True, labels_1d=False):
    """ops.grid_subsample with keys -> the same dict on the host"""
    c = d["c"]
    if c is not None and labels_1d:
        c = c.reshape(-1)
    r = ops.grid_subsample(dev(d["p"], gpu), d["lens"], d["dl"], max_p=max_p, features=dev(d["f"], gpu), labels=dev(c, gpu),
                           reference_order=reference_order, return_keys=True)
    out = dict(p=r[0].cpu().numpy(), lens=r[1], keys=r[-2].cpu().numpy().view(np.uint64), counts=r[-1].cpu().numpy())
    rest = list(r[2:-2])
    if d["f"] is not None:
        out["f"] = rest.pop(0).cpu().numpy()
    if c is not None:
        out["c"] = rest.pop(0).cpu().numpy()
    return out


def assert_same(got, want):
    """lens, keys, counts, points (and features, labels where present): identical bits, identical shapes and types"""
    assert sorted(got) == sorted(want)
    for name in ("lens", "keys", "counts", "p", "f", "c"):
        if name in want:
            g, w = got[name], want[name]
            assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.dtype, w.shape)
            assert np.array_equal(g, w), (name, int((g != w).sum()), np.argwhere(g != w)[:5].tolist())


def sub(d, f=None, c=None):
    """d with other feature / label columns (None = none)"""
    e = dict(d)
    e["f"], e["c"] = f, c
    return e


@pytest.mark.parametrize("name", S.LATTICE_SETS + ["mixed"])
def test_row_counts(gpu, name):
    d = S.dataset(name)
    want = port(d)
    assert want["lens"].tolist() == d["m"]
    assert_same(run(gpu, d), want)


@pytest.mark.parametrize("name", S.ROUNDING_SETS)
def test_rounding(gpu, name):
    d = S.dataset(name)
    assert_same(run(gpu, d), port(d))


def test_wrapped_key(gpu):
    d = S.dataset("wrapped_key")
    want = port(d)
    assert (want["keys"] == S.ALL_ONES).sum() == 1 and want["lens"].tolist() == [61]
    got = run(gpu, d)
    assert (got["keys"] == S.ALL_ONES).sum() == 1
    assert_same(got, want)
    # first-seen order: the wrapped cell belongs to the first point
    first = run(gpu, d, reference_order=False)
    assert first["keys"][0] == S.ALL_ONES
    assert_same(first, _first_seen(d, 0))


# ------------------------------------------------------------------------------------------------------------------
# emission
# ------------------------------------------------------------------------------------------------------------------
_EMIT = {}


def _emit_case(fd, ld):
    if (fd, ld) not in _EMIT:
        e = S.dataset("emit")
        cols = 1 if ld == "1d" else ld
        _EMIT[fd, ld] = sub(e, np.ascontiguousarray(e["f"][:, :fd]), np.ascontiguousarray(e["c"][:, 3 - cols:]))
    return _EMIT[fd, ld]


def _first_seen(d, max_p):
    """the port's rows (all of them) in first-seen order, cut to max_p per element"""
    full = port(d)
    ref = S.cells(d["p"], d["lens"], d["dl"])
    r0 = 0
    for e, m in zip(ref, full["lens"]):                                # the independent key sets are the port's
        assert sorted(e["keys"].tolist()) == sorted(full["keys"][r0:r0 + m].tolist())
        r0 += m
    idx = S.first_seen_rows(ref, full["keys"], full["lens"])
    keep, r0 = [], 0
    for m in full["lens"]:
        keep += list(range(r0, r0 + (min(m, max_p) if max_p > 0 else m)))
        r0 += m
    idx = idx[keep]
    out = {k: v[idx] for k, v in full.items() if k != "lens"}
    out["lens"] = np.asarray([min(m, max_p) if max_p > 0 else m for m in full["lens"]], np.int32)
    return out


@pytest.mark.parametrize("reference_order", [True, False], ids=["reference", "first_seen"])
@pytest.mark.parametrize("max_p", S.EMIT_MAX_P)
@pytest.mark.parametrize("ld", S.EMIT_LD)
@pytest.mark.parametrize("fd", S.EMIT_FD)
def test_emission(gpu, fd, ld, max_p, reference_order):
    d = _emit_case(fd, ld)
    got = run(gpu, d, max_p=max_p, reference_order=reference_order, labels_1d=ld == "1d")
    want = port(d, max_p) if reference_order else _first_seen(d, max_p)
    cols = 1 if ld == "1d" else ld
    assert got["f"].shape[1] == fd and got["c"].shape[1] == cols and got["c"].dtype == np.int32
    assert_same(got, want)


def test_emission_without_optional_outputs(gpu):
    """features alone, labels alone, neither, and no keys: the other outputs do not depend on them"""
    d = _emit_case(3, 2)
    want = port(d)
    for f, c in ((d["f"], None), (None, d["c"]), (None, None)):
        e = sub(d, f, c)
        assert_same(run(gpu, e), {k: v for k, v in want.items() if (k != "f" or f is not None) and (k != "c" or c is not None)})
    r = ops.grid_subsample(dev(d["p"], gpu), d["lens"], d["dl"], features=dev(d["f"], gpu), labels=dev(d["c"], gpu))
    assert len(r) == 4 and np.array_equal(r[0].cpu().numpy(), want["p"]) and np.array_equal(r[1], want["lens"])
    assert np.array_equal(r[2].cpu().numpy(), want["f"]) and np.array_equal(r[3].cpu().numpy(), want["c"])


@pytest.mark.parametrize("name", ["labels_many", "labels_overflow"])
def test_label_histograms(gpu, name):
    d = S.dataset(name)
    want = port(d)
    for reference_order in (True, False):
        got = run(gpu, d, reference_order=reference_order)
        assert_same(got, want if reference_order else _first_seen(d, 0))


def test_crowded_cell(gpu):
    d = S.dataset("crowded")
    want = port(d)
    assert want["counts"].max() == 4096
    assert_same(run(gpu, d), want)
    assert_same(run(gpu, d, reference_order=False), _first_seen(d, 0))


@pytest.mark.parametrize("name", S.SCAN_SETS)
def test_scan_edges(gpu, name):
    d = S.dataset(name)
    assert_same(run(gpu, d), port(d))


# ------------------------------------------------------------------------------------------------------------------
# workspace
# ------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def fresh_workspace(gpu):
    """the calling thread's subsample workspace set aside: the first call inside creates a new one, which is destroyed at the
    end, and the old one comes back"""
    table, key = ops._ws.sub, ops._ws._key(gpu)
    saved = table.pop(key, None)
    try:
        yield
    finally:
        torch.cuda.synchronize()
        made = table.pop(key, None)
        if made is not None:
            _lib.lib().ws_subsample_ws_destroy(made)
        if saved is not None:
            table[key] = saved


def test_workspace_reuse(gpu):
    calls = S.reuse_calls()
    assert len(calls[0]["p"]) == 10000 and len(calls[1]["p"]) == 40
    assert len(calls[1]["lens"]) not in (len(calls[0]["lens"]), len(calls[2]["lens"]))          # nb changes both times
    assert calls[2]["f"] is not None and calls[2]["c"] is not None
    fresh = []
    for d in calls:                                                    # each call first on a workspace of its own
        with fresh_workspace(gpu):
            fresh.append(run(gpu, d))
    with fresh_workspace(gpu):
        for _ in range(2):                                             # large, small, features + labels; and round again
            for d, alone in zip(calls, fresh):
                got = run(gpu, d)
                assert_same(got, alone)
                assert_same(got, port(d))


def test_fill_after_a_failed_plan_is_refused_and_writes_nothing(gpu):
    lib = _lib.lib()
    d = S.dataset("lattice14")
    want = port(d)
    ws = C.c_void_p()
    assert lib.ws_subsample_ws_create(C.byref(ws)) == 0
    try:
        with torch.cuda.device(gpu):
            p = dev(d["p"], gpu)
            out_lens, m = np.zeros(1, np.int32), C.c_int64(-1)

            def plan(points, n):
                hl = np.asarray([n], np.int32)
                return lib.ws_grid_subsample_plan(ws, ptr(points), n, C.c_void_p(hl.ctypes.data), 1, float(np.float32(d["dl"])),
                                                  0, 0, C.c_void_p(out_lens.ctypes.data), C.byref(m), current_stream())

            def fill(out):
                return lib.ws_grid_subsample_fill(ws, None, 0, None, 0, ptr(out), None, None, None, None, current_stream())

            sentinel = torch.full((14, 3), -7.0, device=gpu)
            assert fill(sentinel) == 1 and b"no successful plan" in lib.ws_last_error()      # never planned
            assert plan(p, len(d["p"])) == 0 and m.value == 14
            out = torch.empty((14, 3), device=gpu)
            assert fill(out) == 0 and np.array_equal(out.cpu().numpy(), want["p"])
            assert plan(p[:0], 0) == 4 and m.value == 0 and out_lens[0] == 0                  # WS_ERR_EMPTY
            assert fill(sentinel) == 1 and b"no successful plan" in lib.ws_last_error()
            torch.cuda.synchronize()
            assert (sentinel.cpu().numpy() == -7.0).all()
            assert plan(p, len(d["p"])) == 0 and fill(out) == 0                               # and the workspace recovers
            assert np.array_equal(out.cpu().numpy(), want["p"])
    finally:
        torch.cuda.synchronize()
        lib.ws_subsample_ws_destroy(ws)


# ------------------------------------------------------------------------------------------------------------------
# rotation and the numpy facade
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [64, 65])
def test_rotate_clouds_host_at_the_table_limit(gpu, nb):
    rng = np.random.default_rng(nb)
    lens = rng.integers(1, 30, size=nb).astype(np.int32)
    lens[[0, 7, 8, nb - 1]] = 0                                        # empty elements: first, two in a row, last
    p = rng.normal(size=(int(lens.sum()), 3)).astype(np.float32)
    R = rng.normal(size=(nb, 3, 3)).astype(np.float32)
    want, want_t, i0 = p.copy(), p.copy(), 0
    for b, n in enumerate(lens):
        want[i0:i0 + n] = np.sum(np.expand_dims(p[i0:i0 + n], 2) * R[b], axis=1)             # datasets/common.py:118
        want_t[i0:i0 + n] = np.sum(np.expand_dims(p[i0:i0 + n], 2) * R[b].T, axis=1)         # datasets/common.py:133
        i0 += n
    P = dev(p, gpu)
    assert np.array_equal(ops.rotate_clouds_host(P, lens, R).cpu().numpy(), want)
    assert np.array_equal(ops.rotate_clouds_host(P, lens, R, transpose=True).cpu().numpy(), want_t)
    assert np.array_equal(ops.rotate_clouds(P, dev(lens, gpu), dev(R, gpu)).cpu().numpy(), want)
    # the C entry itself takes 64 elements and refuses 65
    out = torch.empty_like(P)
    rc = _lib.lib().ws_rotate_clouds_host(ptr(P), P.shape[0], C.c_void_p(lens.ctypes.data), nb, C.c_void_p(R.ctypes.data), 0,
                                          ptr(out), current_stream())
    assert rc == (0 if nb == 64 else 2)
    if nb == 64:
        assert np.array_equal(out.cpu().numpy(), want)


def test_facade_with_three_label_columns(gpu):
    from weasal_amd.cpp_wrappers.cpp_subsampling import grid_subsampling as cpp_subsampling
    d = _emit_case(5, 3)
    want = port(d)
    d = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()}      # writable copies for the facade
    p, l, f, c = cpp_subsampling.subsample_batch(d["p"].astype(np.float64), list(d["lens"]), features=d["f"], classes=d["c"],
                                                 sampleDl=d["dl"])
    for a, dtype, w in ((p, np.float32, want["p"]), (l, np.int32, want["lens"]), (f, np.float32, want["f"]), (c, np.int32, want["c"])):
        assert isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == w.shape and np.array_equal(a, w)
    assert c.shape == (len(p), 3)
    # single-cloud form on the first element: points, features, classes (wrapper.cpp:338-566)
    n0 = int(d["lens"][0])
    one = sub(d, d["f"][:n0], d["c"][:n0])
    one["p"], one["lens"] = d["p"][:n0], d["lens"][:1]
    w1 = port(one)
    p1, f1, c1 = cpp_subsampling.subsample(one["p"], features=one["f"], classes=one["c"], sampleDl=d["dl"])
    assert np.array_equal(p1, w1["p"]) and np.array_equal(f1, w1["f"]) and np.array_equal(c1, w1["c"]) and c1.shape == (len(p1), 3)
    # one-dimensional classes come back as a column
    w2 = port(sub(one, None, one["c"][:, :1]))
    p2, c2 = cpp_subsampling.subsample(one["p"], classes=one["c"][:, 0], sampleDl=d["dl"])
    assert c2.shape == (len(p2), 1) and c2.dtype == np.int32 and np.array_equal(c2, w2["c"]) and np.array_equal(p2, w2["p"])
