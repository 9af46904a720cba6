"""GPU: the exact nearest-neighbour search (ws_nearest_neighbors -> ops.nearest_neighbors -> tester.nearest_projection;
DESIGN.md section 22).  Every case is held to tests/nearest_ref.py -- the float64 brute force with the tree's recipe -- for
EQUALITY of the indices and bit-equality of the squared distances; the golden batch also to sklearn's KDTree itself
(tests/golden/g22_nearest.npz).  The non-finite queries come last in the file."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import golden
from nearest_ref import nearest_ref

pytestmark = pytest.mark.gpu


def run(gpu, q, s, ql, sl, cell=0.0, dtype=torch.int32, status=None):
    from weasal_amd import ops
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)).to(gpu)
    idx, d2 = ops.nearest_neighbors(dev(q), dev(s), ql, sl, cell=cell, dtype=dtype, return_d2=True, status=status)
    assert idx.dtype == dtype and d2.dtype == torch.float64 and idx.shape == d2.shape == (len(np.reshape(q, (-1, 3))),)
    return idx.cpu().numpy(), d2.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


def hold(gpu, q, s, ql, sl, cells=(0.0,)):
    """every cell size gives the reference's indices and the reference's float64 bits; -> the reference"""
    want_i, want_d = nearest_ref(q, s, ql, sl)
    for cell in cells:
        got_i, got_d = run(gpu, q, s, ql, sl, cell)
        bad = np.nonzero(got_i != want_i)[0]
        assert len(bad) == 0, (cell, bad[:8], got_i[bad[:8]], want_i[bad[:8]])
        assert same_bits(got_d, want_d), cell
    return want_i, want_d


@functools.lru_cache(maxsize=None)
def golden_ref():
    g = golden("g22_nearest.npz")
    return nearest_ref(g["queries"], g["supports"], g["q_lens"], g["s_lens"])


def test_golden_batch_equals_the_tree_and_the_reference(gpu):
    g = golden("g22_nearest.npz")
    q, s, ql, sl = g["queries"], g["supports"], g["q_lens"], g["s_lens"]
    want_i, want_d = golden_ref()
    i32, d32 = run(gpu, q, s, ql, sl, dtype=torch.int32)
    i64, d64 = run(gpu, q, s, ql, sl, dtype=torch.int64)
    assert np.array_equal(i32.astype(np.int64), i64) and same_bits(d32, d64)
    free = g["tie_free"]
    assert np.array_equal(i32[free], g["idx"][free])                      # sklearn's KDTree.query
    assert np.array_equal(i64, want_i) and same_bits(d64, want_d)         # all rows
    again_i, again_d = run(gpu, q, s, ql, sl, dtype=torch.int64)
    assert np.array_equal(again_i, i64) and same_bits(again_d, d64)


def test_result_does_not_depend_on_the_cell(gpu):
    g = golden("g22_nearest.npz")
    dl = float(g["dl"])
    want_i, want_d = golden_ref()
    for cell in (0.0, dl / 8, dl, 64 * dl):          # library's choice; small cells; the ordinary case; one cell, runs > 64
        got_i, got_d = run(gpu, g["queries"], g["supports"], g["q_lens"], g["s_lens"], cell)
        assert np.array_equal(got_i, want_i) and same_bits(got_d, want_d), cell


def test_far_and_outside_queries(gpu):
    g = golden("g22_nearest.npz")
    dl = float(g["dl"])
    s = g["supports"][:int(g["s_lens"][0])]
    lo, hi = s.min(0).astype(np.float64), s.max(0).astype(np.float64)
    rng = np.random.default_rng(3)
    q = rng.uniform(lo, hi, (300, 3))
    dirs = [(a, sg) for a in range(3) for sg in (-1, 1)] + [(None, -1), (None, 1)]        # six faces, two diagonals
    for i in range(300):
        (axis, sign), mag = dirs[i % 8], (0.5, 10.0, 1000.0)[(i // 8) % 3]
        for a in (range(3) if axis is None else (axis,)):
            q[i, a] = (hi[a] + mag * dl) if sign > 0 else (lo[a] - mag * dl)
    q = q.astype(np.float32)
    assert np.all(np.any((q < lo) | (q > hi), axis=1))
    hold(gpu, q, s, [300], [len(s)], cells=(0.0, dl, dl / 4))
    # a slab cloud queried from above, next to the far queries in one batch
    slab = (rng.uniform(0, 1, (1500, 3)) * np.array([40.0, 40.0, 0.2])).astype(np.float32)
    above = (rng.uniform(0, 1, (200, 3)) * np.array([40.0, 40.0, 0.0]) + np.array([0, 0, 1.0]) *
             np.repeat([0.3, 2.0, 9.0, 30.0], 50)[:, None]).astype(np.float32)
    hold(gpu, np.concatenate([q, above]), np.concatenate([s, slab]), [300, 200], [len(s), 1500], cells=(0.0, 0.7))


def test_exact_ties_go_to_the_smallest_index(gpu):
    rng = np.random.default_rng(4)
    lat = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3)
    s = np.concatenate([lat, lat[rng.choice(len(lat), 40, replace=False)]])
    s = (s[rng.permutation(len(s))] * 0.25).astype(np.float32)
    q = (np.stack(np.meshgrid(*[np.arange(11)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.125).astype(np.float32)
    want_i, want_d = hold(gpu, q, s, [len(q)], [len(s)], cells=(0.0, 0.25, 0.1))
    d2 = ((q[:, None, :].astype(np.float64) - s[None].astype(np.float64)) ** 2).sum(-1)
    tied = (d2 == d2.min(1, keepdims=True)).sum(1)
    assert (tied >= 2).sum() > 1000 and (tied >= 8).sum() > 50                      # the case is about ties
    assert np.array_equal(want_i, (d2 == d2.min(1, keepdims=True)).argmax(1))         # smallest index of the minimal set


def test_batch_elements_are_isolated(gpu):
    rng = np.random.default_rng(5)
    sa = rng.uniform(0, 1, (90, 3)).astype(np.float32)                   # element 0: supports in a corner ...
    qa = rng.uniform(0, 3, (60, 3)).astype(np.float32)                   # ... queries all over the place
    qb = rng.uniform(0, 3, (25, 3)).astype(np.float32)                   # element 1: no supports
    sc = rng.uniform(0, 3, (400, 3)).astype(np.float32)                  # element 2: no queries, supports everywhere
    q, s = np.concatenate([qa, qb]), np.concatenate([sa, sc])
    ql, sl = [60, 25, 0], [90, 0, 400]
    want_i, want_d = hold(gpu, q, s, ql, sl, cells=(0.0, 0.3))
    assert np.all(want_i[:60] < 90) and np.all(want_i[60:] == 490) and np.all(np.isinf(want_d[60:]))
    all_i, _ = nearest_ref(q[:60], s, [60], [490])
    assert (all_i >= 90).sum() > 30                                       # a closer support of element 2 must not win
    # a single support
    one = np.array([[1.5, -2.0, 0.25]], np.float32)
    want_i, _ = hold(gpu, qa, one, [60], [1], cells=(0.0, 1.0))
    assert np.all(want_i == 0)
    # no supports at all
    got_i, got_d = run(gpu, qa, np.zeros((0, 3), np.float32), [60], [0])
    assert np.all(got_i == 0) and np.all(np.isposinf(got_d))


def test_more_elements_than_the_launch_table_holds(gpu):
    """nb > 48: the per-element table is staged through a copy instead of a kernel argument"""
    rng = np.random.default_rng(6)
    nb = 50
    ql, sl = rng.integers(1, 30, nb), rng.integers(1, 20, nb)
    sl[7] = 0
    ql[11] = 0
    q = rng.uniform(-2, 2, (int(ql.sum()), 3)).astype(np.float32)
    s = rng.uniform(-1, 1, (int(sl.sum()), 3)).astype(np.float32)
    want_i, _ = hold(gpu, q, s, ql, sl, cells=(0.0, 0.5))
    assert (want_i == len(s)).sum() == ql[7]


def test_self_query(gpu):
    from weasal_amd import ops
    g = golden("g22_nearest.npz")
    dup = g["supports"][::7]
    p = np.concatenate([g["supports"], dup])                              # duplicates behind their originals
    lens = [len(p)]
    P = torch.from_numpy(p).to(gpu)
    idx, d2 = ops.nearest_neighbors(P, P, lens, lens, return_d2=True)      # the same tensor: walked in cell order
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    assert np.all(d2 == 0) and np.all(idx <= np.arange(len(p))) and np.all(p[idx] == p)
    assert (idx < np.arange(len(p))).sum() == len(dup)
    want_i, want_d = nearest_ref(p, p, lens, lens)
    assert np.array_equal(idx, want_i) and same_bits(d2, want_d)


def test_contract_is_checked_before_anything_is_queued(gpu):
    from weasal_amd import _lib
    lib = _lib.lib()
    OK, INVALID = 0, 1
    one, null = C.c_void_p(16), C.c_void_p(None)                          # never dereferenced: validation fails first
    l4, l3, lneg, l0 = ((C.c_int32 * 1)(v) for v in (4, 3, -1, 0))
    hp = lambda a: C.cast(a, C.c_void_p)
    ws = C.c_void_p()
    assert lib.ws_neighbors_ws_create(C.byref(ws)) == 0
    before = lib.ws_launch_count()

    def call(ws=ws, q=one, nq=4, s=one, ns=4, ql=l4, sl=l4, nb=1, cell=0.0, o32=one, o64=null, d2=null, st=null):
        return lib.ws_nearest_neighbors(ws, q, nq, s, ns, hp(ql), hp(sl), nb, cell, o32, o64, d2, st, None), lib.ws_last_error()
    for over in ({"ws": null}, {"q": null}, {"s": null}):
        rc, msg = call(**over)
        assert rc == INVALID and b"NULL" in msg, over
    for name in ("ql", "sl"):
        rc = lib.ws_nearest_neighbors(ws, one, 4, one, 4, null if name == "ql" else hp(l4), null if name == "sl" else hp(l4), 1,
                                      0.0, one, null, null, null, None)
        assert rc == INVALID and b"NULL" in lib.ws_last_error()
    for over in ({"o32": one, "o64": one}, {"o32": null, "o64": null}):
        rc, msg = call(**over)
        assert rc == INVALID and b"exactly one" in msg, over
    for over in ({"ql": lneg, "nq": -1}, {"ql": lneg}, {"sl": lneg}, {"nq": -4}, {"ns": -4}, {"nb": 0}):
        assert call(**over)[0] == INVALID, over
    for over in ({"ql": l3}, {"sl": l3}, {"nq": 5}, {"ns": 3}):
        rc, msg = call(**over)
        assert rc == INVALID and b"do not sum" in msg, over
    assert call(cell=-1.0)[0] == INVALID and call(cell=float("inf"))[0] == INVALID
    assert call(q=null, nq=0, ql=l0)[0] == OK                              # nq == 0: fine, and nothing to do
    assert call(q=null, nq=0, ql=l0, s=null, ns=0, sl=l0)[0] == OK
    assert lib.ws_launch_count() == before                                  # none of this reached the device
    lib.ws_neighbors_ws_destroy(ws)


def test_projection_default_equals_the_radius_route_and_the_tree(gpu):
    from weasal_amd import tester
    g = golden("g11_tester.npz")
    full, sub, dl = g["full"], g["sub"], float(g["dl"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    new = tester.nearest_projection(dev(full), dev(sub))
    old = tester.nearest_projection(dev(full), dev(sub), dl * 3 ** 0.5)
    assert new.dtype == old.dtype == torch.int32 and new.shape == old.shape == (len(full),)
    new, old = new.cpu().numpy(), old.cpu().numpy()
    # the float32 route's two best distances, with its recipe (ws_grid.h: ref_d2)
    decided = np.empty(len(full), bool)
    for a in range(0, len(full), 1024):
        d = full[a:a + 1024, None, :] - sub[None]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert d2.dtype == np.float32
        two = np.partition(d2, 1, axis=1)[:, :2]
        decided[a:a + 1024] = two[:, 0] != two[:, 1]
    print("rows the float32 route decides by index:", int((~decided).sum()), "of", len(full),
          "; routes differ on", int((new != old).sum()))
    assert np.array_equal(new[decided], old[decided])
    # the golden's projection is the tree's: equal on every row where the two nearest float64 distances differ, and on a
    # tied row the smaller index of two equal float64 distances
    proj = g["proj"].astype(np.int64)
    differ = np.nonzero(new != proj)[0]
    if len(differ):
        f, s = full[differ].astype(np.float64), sub.astype(np.float64)
        da, db = f - s[new[differ]], f - s[proj[differ]]
        assert np.array_equal((da[:, 0] * da[:, 0] + da[:, 1] * da[:, 1]) + da[:, 2] * da[:, 2],
                              (db[:, 0] * db[:, 0] + db[:, 1] * db[:, 1]) + db[:, 2] * db[:, 2])
        assert np.all(new[differ] < proj[differ])


def test_non_finite_queries_get_ns_and_the_status_bit(gpu):
    """LAST: the shell loop of nn_exact_kernel is bounded by max(nx, ny, nz) and a non-finite query never enters it."""
    from weasal_amd import ops
    g = golden("g22_nearest.npz")
    s = g["supports"][:int(g["s_lens"][0])]
    q = g["queries"][:204].copy()
    rows = [17, 64, 130, 203]
    q[17, 0] = np.nan
    q[64, 1] = np.inf
    q[130, 2] = -np.inf
    q[203] = np.nan
    status = torch.zeros(1, dtype=torch.int32, device=gpu)
    got_i, got_d = run(gpu, q, s, [204], [len(s)], status=status)
    want_i, want_d = nearest_ref(q, s, [204], [len(s)])
    assert np.all(want_i[rows] == len(s)) and (want_i != len(s)).sum() == 200
    assert np.array_equal(got_i, want_i) and same_bits(got_d, want_d)
    assert int(status.item()) == ops.NN_STATUS_NONFINITE_QUERY
    clean = torch.zeros(1, dtype=torch.int32, device=gpu)
    keep = np.setdiff1d(np.arange(204), rows)
    got2_i, got2_d = run(gpu, q[keep], s, [200], [len(s)], status=clean)
    assert int(clean.item()) == 0 and np.array_equal(got2_i, want_i[keep]) and same_bits(got2_d, want_d[keep])
