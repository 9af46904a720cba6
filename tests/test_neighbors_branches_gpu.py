"""Every launch branch of the radius search (weasal_amd/csrc/neighbors.hip) against the brute-force reference of
oracle/neighbors_ref.py: every query against every support of its element, the reference's float32 distance recipe, rows
ordered by the key (d2 bits << 32 | index).  Everything is integer-exact; every comparison is array_equal.

Which kernel ran is read from the library (ws_radius_neighbors_last_fills -> ws_radius_neighbors_fill_variant) and held to
oracle.neighbors_ref.fill_plan; tests/test_neighbors_branches_cpu.py holds that mirror to the library's reporter, the
reference to the CPU oracles, and asserts that the tables below reach every launch form and straddle every step:
row counts 128/129, 576/577, 704/705, 1024/1025, 2048/2049 and asynchronous widths 128/129, 461/462, 563/564.

Data (all at most ~2400 points, the "long" sets apart):
  uniform      two overlapping spheres with an empty element between them, rows <= 128
  lattice      9^3 points at spacing 0.25, shuffled: r = 0.5 / 0.75 / 1.0 give rows of 27 / 93 / 251; exact d2 ties everywhere,
               d = r occurs exactly (and is excluded)
  clump<m>     300 scattered points + m points inside a ball of radius 0.24: at r = 0.5 every clump row holds exactly m
  coincident<n> n copies of one point + background: n keys with d2 = 0 in one bucket, ranked by index alone
  near         three elements, one per axis: supports at k 1.75, queries at +-0.5, +-(0.5 - 2^-13), 0.5 + 2^-13 from them
  line         200 points over 1500 units in x: the grid's cell has to grow
  degenerate   one support; supports without queries; queries without supports; an empty element; two supports; coplanar
               supports with queries far outside their box
  offset       clouds near (1000, 2000, 50)
  many         70 overlapping elements of 20 .. 60 points (beyond the 48-entry argument table)
  long_q / long_self / tiny<n>   16500 queries (past the 4096-workgroup cap), 4200 self-queried points (past the 1024 cap of the
               asynchronous entries), 1 / 3 / 4 / 5 / 33 queries (the grid rounding of ws_block_range)
The tables are plain data; every case runs twice and must repeat its bits.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from conftest import sphere
from oracle import neighbors_ref as R
from weasal_amd import _lib, ops
from weasal_amd._lib import check, current_stream, ptr

pytestmark = pytest.mark.gpu

RADIUS = 0.5
CLUMP_M = (128, 129, 576, 577, 704, 705, 1024, 1025, 2048, 2049)
CLUMP_R, CLUMP_AWAY, SCATTER_N = 0.24, 20.0, 300
LATTICE_N, LATTICE_STEP = 9, 0.25
LATTICE_ROWS = {0.5: 27, 0.75: 93, 1.0: 251}
NEAR_K, NEAR_PITCH, NEAR_EPS = 143, 1.75, 2.0 ** -13
NEAR_OFFSETS = (0.5, -0.5, 0.5 - NEAR_EPS, -(0.5 - NEAR_EPS), 0.5 + NEAR_EPS)
LINE_N, LINE_LENGTH = 200, 1500.0
COINCIDENT_AT = (0.3, -0.2, 0.1)
TINY_NQ = (1, 3, 4, 5, 33)
DT = {"i32": torch.int32, "i64": torch.int64}


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _set(s, sl, q=None, ql=None, **extra):
    s = np.ascontiguousarray(s, dtype=np.float32)
    d = dict(s=s, sl=np.asarray(sl, np.int32), self_query=q is None, **extra)
    d["q"] = s if q is None else np.ascontiguousarray(q, dtype=np.float32)
    d["ql"] = d["sl"] if q is None else np.asarray(ql, np.int32)
    return d


def _make(name):
    rng = _rng(name)
    if name == "uniform":
        return _set(np.concatenate([sphere(rng, 700, 2.0), sphere(rng, 500, 2.0, center=(1, 0, 0))]), [700, 0, 500])
    if name == "uniform_x":                                       # other queries over the supports of "uniform"
        q = np.concatenate([sphere(rng, 300, 2.2), sphere(rng, 200, 2.2, center=(1, 0, 0))])
        return _set(_make("uniform")["s"], [700, 0, 500], q, [300, 0, 200])
    if name == "lattice":
        g = np.arange(LATTICE_N, dtype=np.float32) * np.float32(LATTICE_STEP)
        pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        return _set(pts[rng.permutation(len(pts))], [len(pts)])
    if name == "lattice_mid":                                     # queries at the centres of the lattice's cubes: 8 nearest, tied
        s = _make("lattice")["s"]
        g = (np.arange(LATTICE_N - 1, dtype=np.float32) + np.float32(0.5)) * np.float32(LATTICE_STEP)
        q = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        return _set(s, [len(s)], q[rng.permutation(len(q))], [len(q)])
    if name.startswith("clump"):
        m = int(name[5:])
        pts = np.concatenate([sphere(rng, SCATTER_N, 3.0), sphere(rng, m, CLUMP_R, center=(CLUMP_AWAY, 0, 0))])
        perm = rng.permutation(len(pts))
        return _set(pts[perm], [len(pts)], in_clump=perm >= SCATTER_N, m=m)
    if name.startswith("coincident"):
        n = int(name[10:])
        pts = np.concatenate([sphere(rng, SCATTER_N, 3.0), np.tile(np.asarray(COINCIDENT_AT, np.float32), (n, 1))])
        perm = rng.permutation(len(pts))
        return _set(pts[perm], [len(pts)], copies=perm >= SCATTER_N, n=n)
    if name == "near":
        s, q = [], []
        for axis in range(3):
            x = np.arange(NEAR_K, dtype=np.float64) * NEAR_PITCH
            sa = np.zeros((NEAR_K, 3))
            sa[:, axis] = x
            qa = np.zeros((NEAR_K * len(NEAR_OFFSETS), 3))
            qa[:, axis] = (x[:, None] + np.asarray(NEAR_OFFSETS)[None, :]).reshape(-1)
            assert np.array_equal(qa.astype(np.float32).astype(np.float64), qa)      # exactly representable
            s.append(sa)
            q.append(qa[rng.permutation(len(qa))])
        return _set(np.concatenate(s), [NEAR_K] * 3, np.concatenate(q), [NEAR_K * len(NEAR_OFFSETS)] * 3)
    if name == "line":
        x = np.concatenate([[0.0, LINE_LENGTH], rng.uniform(0, LINE_LENGTH, size=LINE_N // 2 - 2)])
        base = np.stack([x, rng.uniform(-0.2, 0.2, size=x.size), rng.uniform(-0.2, 0.2, size=x.size)], 1)
        mate = base + rng.uniform(-0.15, 0.15, size=base.shape)
        mate[:2, 0] = base[:2, 0]                                 # the ends stay the ends
        pts = np.concatenate([base, mate])
        return _set(pts[rng.permutation(len(pts))], [len(pts)])
    if name == "degenerate":
        plane = np.concatenate([rng.uniform(0, 4, size=(200, 2)), np.full((200, 1), 2.0)], 1)
        s = [[(1, 1, 1)], rng.uniform(-1, 1, size=(40, 3)), np.zeros((0, 3)), np.zeros((0, 3)), [(0, 0, 0), (0.3, 0, 0)], plane]
        near_plane = np.concatenate([rng.uniform(0, 4, size=(60, 2)), rng.uniform(1.7, 2.3, size=(60, 1))], 1)
        far = [(10, 10, 2), (-3, 2, 2), (2, 2, 9), (2, 2, -9), (3e5, 2, 2), (-1e7, 2, 2), (2, 5.6, 2), (2, -1.6, 2)]
        q = [[(1, 1, 1), (1.2, 1, 1), (1.49, 1, 1), (1.5, 1, 1), (50, 50, 50), (-50, 1, 1), (1, 1, 2.5)], np.zeros((0, 3)),
             rng.uniform(-1, 1, size=(7, 3)), np.zeros((0, 3)), [(0.1, 0, 0), (0.15, 0, 0), (5, 0, 0), (0, 0, 0.49), (0.3, 0.5, 0)],
             np.concatenate([near_plane, far])]
        s, q = [np.asarray(a, np.float64).reshape(-1, 3) for a in s], [np.asarray(a, np.float64).reshape(-1, 3) for a in q]
        return _set(np.concatenate(s), [len(a) for a in s], np.concatenate(q), [len(a) for a in q], far=len(far))
    if name == "offset":
        return _set(np.concatenate([sphere(rng, 500, 1.5, center=(1000, 2000, 50)), sphere(rng, 400, 1.5, center=(1003, 2000, 50))]),
                    [500, 400])
    if name == "many":
        lens = rng.integers(20, 61, size=70)
        return _set(np.concatenate([sphere(rng, int(n), 0.8) for n in lens]), lens)
    if name == "many_x":
        sl = _make("many")["sl"]
        ql = rng.integers(1, 9, size=70)
        return _set(_make("many")["s"], sl, np.concatenate([sphere(rng, int(n), 0.9) for n in ql]), ql)
    if name == "long_q":
        s = np.concatenate([sphere(rng, 900, 3.0), sphere(rng, 600, 3.0)])
        q = np.concatenate([sphere(rng, 9000, 3.2), sphere(rng, 7500, 3.2)])
        return _set(s, [900, 600], q, [9000, 7500])
    if name == "long_self":
        return _set(np.concatenate([sphere(rng, 2500, 3.5), sphere(rng, 1700, 3.0)]), [2500, 1700])
    if name.startswith("tiny"):
        nq = int(name[4:])
        return _set(sphere(rng, 300, 1.5), [300], sphere(rng, nq, 1.5), [nq])
    if name == "nowhere":                                         # no query has a neighbour
        return _set(_make("uniform")["s"], [700, 0, 500], _make("uniform_x")["q"] + np.float32(100), [300, 0, 200])
    raise KeyError(name)


_SETS, _REFS, _DEV = {}, {}, {}


def dataset(name):
    if name not in _SETS:
        _SETS[name] = _make(name)
    return _SETS[name]


def reference(name, radius=RADIUS):
    """(keys, counts) of oracle.neighbors_ref.brute_keys, computed once per (set, radius) and never changed"""
    if (name, radius) not in _REFS:
        d = dataset(name)
        keys, counts = R.brute_keys(d["q"], d["s"], d["ql"], d["sl"], radius)
        keys.setflags(write=False)
        counts.setflags(write=False)
        _REFS[name, radius] = (keys, counts)
    return _REFS[name, radius]


def max_count(name, radius=RADIUS):
    return int(reference(name, radius)[1].max())


# ------------------------------------------------------------------------------------------------------------------
# case tables (plain data)
# ------------------------------------------------------------------------------------------------------------------
# plan + fill, full width: (set, radius)
PLAN_FILL = [("uniform", 0.5), ("uniform_x", 0.5), ("lattice", 0.5), ("lattice", 0.75), ("lattice", 1.0), ("lattice_mid", 0.5)] + \
            [("clump%d" % m, 0.5) for m in CLUMP_M if m <= 2048] + \
            [("coincident600", 0.5), ("coincident100", 0.5), ("near", 0.5), ("line", 0.5), ("degenerate", 0.5), ("offset", 0.5),
             ("many", 0.5), ("many_x", 0.5), ("long_q", 0.4)] + [("tiny%d" % n, 0.5) for n in TINY_NQ]

# synchronous one-pass search: (set, radius, width, note)
SEARCH = [
    ("lattice", 0.75, 1, "width 1"), ("lattice", 0.75, 50, "below the count: truncation, among ties"),
    ("lattice", 0.75, 93, "equal to the maximum"), ("lattice", 0.75, 120, "above it: trimmed"),
    ("clump128", 0.5, 128, "128 slab, full"), ("clump129", 0.5, 128, "re-run into 576"), ("clump129", 0.5, 100, "re-run into 576"),
    ("clump576", 0.5, 64, "re-run into 576, full"), ("clump577", 0.5, 128, "re-run into 704"), ("clump704", 0.5, 7, "re-run into 704, full"),
    ("clump705", 0.5, 64, "re-run into 1024"), ("clump1024", 0.5, 5, "a narrow width on the 1024 slab, full"),
    ("clump1025", 0.5, 128, "width <= 128, re-run into 2048"), ("clump2048", 0.5, 1, "width 1 on the 2048 slab, full"),
    ("clump128", 0.5, 129, "wide kernel on short rows, trimmed"), ("clump576", 0.5, 200, "1024 slab from the start"),
    ("clump1024", 0.5, 1024, "1024 slab, full, equal"), ("clump1025", 0.5, 300, "width > 128, re-run into 2048"),
    ("clump2048", 0.5, 2048, "2048 slab, equal"), ("clump2048", 0.5, 2100, "2048 slab, trimmed"),
    ("lattice", 1.0, 251, "ties on the 1024 slab"), ("lattice", 1.0, 130, "truncation among ties on the 1024 slab"),
    ("coincident600", 0.5, 600, "600 equal d2 in one bucket"), ("coincident600", 0.5, 128, "re-run into 704"),
    ("coincident600", 0.5, 1, "width 1"), ("coincident100", 0.5, 128, "100 equal d2 in the 128 slab"),
    ("near", 0.5, 4, "d = r and d = r -+ 2^-13"), ("line", 0.5, 8, "grown cells"), ("degenerate", 0.5, 16, "degenerate elements"),
    ("offset", 0.5, 64, "far from the origin"), ("many", 0.5, 40, "70 elements"), ("many_x", 0.5, 40, "70 elements, other queries"),
    ("long_q", 0.4, 16, "past the 4096-workgroup cap"), ("uniform", 0.5, 128, "empty element in the middle"),
    ("uniform_x", 0.5, 20, "other queries"),
] + [("tiny%d" % n, 0.5, 30, "%d queries" % n) for n in TINY_NQ]

# rows of 2049: (entry, width)
UNSUPPORTED = [("plan_fill", 0), ("search", 128), ("search", 200), ("async", 564)]

# DeferredSearches: (set, radius, width, ws_nb_wide_caps)
DEFERRED = [
    ("lattice", 0.75, 128, 1), ("lattice", 0.75, 50, 1), ("clump128", 0.5, 128, 1), ("clump129", 0.5, 128, 1),
    ("clump128", 0.5, 129, 1), ("clump128", 0.5, 129, 0), ("clump576", 0.5, 461, 1), ("clump577", 0.5, 461, 1),
    ("clump704", 0.5, 462, 1), ("clump704", 0.5, 563, 1), ("clump705", 0.5, 563, 1), ("clump705", 0.5, 462, 0),
    ("clump1024", 0.5, 564, 1), ("clump1025", 0.5, 564, 1), ("clump1025", 0.5, 461, 0), ("clump577", 0.5, 128, 1),
    ("coincident600", 0.5, 500, 1), ("coincident100", 0.5, 128, 1), ("lattice", 1.0, 251, 1), ("lattice", 1.0, 200, 1),
    ("near", 0.5, 4, 1), ("line", 0.5, 8, 1), ("degenerate", 0.5, 16, 1), ("offset", 0.5, 40, 1), ("many", 0.5, 30, 1),
    ("many_x", 0.5, 30, 1), ("long_self", 0.5, 30, 1), ("uniform", 0.5, 40, 1), ("uniform_x", 0.5, 40, 1), ("tiny33", 0.5, 30, 1),
]

# the asynchronous entry through the C ABI, int32 and int64 rows: (set, radius, width, ws_nb_wide_caps)
ASYNC_RAW = [("lattice", 0.75, 50, 1), ("clump129", 0.5, 128, 1), ("clump577", 0.5, 461, 1), ("clump704", 0.5, 563, 1),
             ("clump1024", 0.5, 564, 1), ("clump128", 0.5, 129, 0), ("uniform", 0.5, 40, 1), ("long_self", 0.5, 30, 1)]

# nearest only: (set, radius)
NEAREST = [("uniform", 0.5), ("uniform_x", 0.5), ("lattice", 0.5), ("lattice_mid", 0.5), ("near", 0.5), ("degenerate", 0.5),
           ("coincident600", 0.5), ("many", 0.5), ("many_x", 0.5), ("long_self", 0.5), ("line", 0.5), ("nowhere", 0.5)] + \
          [("tiny%d" % n, 0.5) for n in TINY_NQ]

# self-query through a clone of the tensor (no cell-order walk): (set, radius, entry, width)
CLONE = [("uniform", 0.5, "plan_fill", 0), ("lattice", 1.0, "plan_fill", 0), ("clump577", 0.5, "search", 300),
         ("coincident600", 0.5, "async", 500), ("clump129", 0.5, "async", 100), ("many", 0.5, "search", 40)]


def case_plans():
    """(entry, output type, plan) of every search the tables above make; the plan is oracle.neighbors_ref.fill_plan's"""
    out = []
    for name, r in PLAN_FILL:
        for t in DT:
            out.append(("plan_fill", t, tuple(R.fill_plan("plan_fill", 0, max_count(name, r), 1, t == "i32"))))
    for name, r, w, _ in SEARCH:
        for t in DT:
            out.append(("search", t, tuple(R.fill_plan("search", w, max_count(name, r), 1, t == "i32"))))
    for entry, w in UNSUPPORTED:
        for t in DT if entry != "async" else ("i64",):
            out.append((entry, t, tuple(R.fill_plan(entry, w, 2049, 1, t == "i32"))))
    for name, r, w, wide in DEFERRED:
        out.append(("async", "i64", tuple(R.fill_plan("async", w, max_count(name, r), wide, False))))
    for name, r, w, wide in ASYNC_RAW:
        for t in DT:
            out.append(("async", t, tuple(R.fill_plan("async", w, max_count(name, r), wide, t == "i32")[:1])))
    for name, r in NEAREST:
        for t in DT:
            out.append(("nearest", t, tuple(R.fill_plan("nearest", 1, max_count(name, r), 1, t == "i32"))))
    return out


# ------------------------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------------------------
def _dev(gpu, name):
    if name not in _DEV:
        d = dataset(name)
        s = torch.from_numpy(d["s"]).to(gpu)
        _DEV[name] = (s if d["self_query"] else torch.from_numpy(d["q"]).to(gpu), s)
    return _DEV[name]


@pytest.fixture(autouse=True)
def _restore_wide_caps():
    """a search that overflows its slab switches the process to 1024-entry slabs (ops.widen_async_slabs): put the switch back"""
    flag = C.c_int.in_dll(_lib.lib(), "ws_nb_wide_caps")
    saved = flag.value
    yield
    flag.value = saved


def _set_wide_caps(v):
    C.c_int.in_dll(_lib.lib(), "ws_nb_wide_caps").value = v


def ran(gpu, out_i32, beside=False):
    """names of the fill launches the last entry on this thread's workspace made (the library's record and reporter)"""
    lib = _lib.lib()
    caps, n = (C.c_int32 * 8)(), C.c_int32(0)
    check(lib.ws_radius_neighbors_last_fills(ops._ws.neighbors(gpu), caps, 8, C.byref(n)))
    assert 0 <= n.value <= 8
    names = []
    for c in caps[:n.value]:
        buf = C.create_string_buffer(96)
        check(lib.ws_radius_neighbors_fill_variant(c, int(out_i32), int(beside), buf, 96))
        names.append(buf.value.decode())
    return names


def _np(t):
    return t.cpu().numpy()


def _want_rows(name, r, width):
    """rows of the final matrix of a search at `width`: the count's width when that is smaller"""
    keys, counts = reference(name, r)
    return R.rows(keys, counts, min(width, int(counts.max())), len(dataset(name)["s"]))


def _sync_search(gpu, name, r, width, t, q=None):
    d = dataset(name)
    qd, sd = _dev(gpu, name)
    out, counts = ops.radius_neighbors(qd if q is None else q, sd, d["ql"], d["sl"], r, limit=width or None, dtype=DT[t],
                                       return_counts=True)
    return out, counts


@pytest.mark.parametrize("t", list(DT))
@pytest.mark.parametrize("name,r", PLAN_FILL, ids=["%s-r%g" % c for c in PLAN_FILL])
def test_plan_fill(gpu, name, r, t):
    keys, counts = reference(name, r)
    mc = int(counts.max())
    want = R.rows(keys, counts, mc, len(dataset(name)["s"]))
    plan = R.fill_plan("plan_fill", 0, mc, 1, t == "i32")
    got = []
    for _ in range(2):
        out, cnt = _sync_search(gpu, name, r, 0, t)
        names = ran(gpu, t == "i32")
        print(name, r, t, names)
        assert names == plan
        assert out.dtype == DT[t] and np.array_equal(_np(out), want)
        assert np.array_equal(_np(cnt), counts)
        got.append(_np(out))
    assert np.array_equal(got[0], got[1])


@pytest.mark.parametrize("t", list(DT))
@pytest.mark.parametrize("name,r,width,note", SEARCH, ids=["%s-r%g-w%d" % c[:3] for c in SEARCH])
def test_search(gpu, name, r, width, note, t):
    keys, counts = reference(name, r)
    want = _want_rows(name, r, width)
    plan = R.fill_plan("search", width, int(counts.max()), 1, t == "i32")
    got = []
    for _ in range(2):
        out, cnt = _sync_search(gpu, name, r, width, t)
        names = ran(gpu, t == "i32")
        print(name, r, width, t, note, names)
        assert names == plan
        assert out.dtype == DT[t] and np.array_equal(_np(out), want)
        assert np.array_equal(_np(cnt), counts)
        got.append(_np(out))
    assert np.array_equal(got[0], got[1])


@pytest.mark.parametrize("t", list(DT))
def test_rows_of_2049_are_refused_and_the_workspace_recovers(gpu, t):
    assert max_count("clump2049") == 2049
    for entry, width in UNSUPPORTED:
        if entry == "async" and t == "i32":
            continue
        plan = R.fill_plan(entry, width, 2049, 1, t == "i32")
        assert plan[-1] == R.UNSUPPORTED
        with pytest.raises(_lib.WeasalHipError, match="status 2.*2049 exceeds the 2048-entry sort slab"):
            if entry == "async":
                d = ops.DeferredSearches(gpu)
                qd, sd = _dev(gpu, "clump2049")
                d.add(qd, sd, [2349], [2349], RADIUS, width)
                assert ran(gpu, False, beside=True) == plan[:1]
                plan = plan[1:]
                d.finish()
            else:
                _sync_search(gpu, "clump2049", RADIUS, width, t)
        names = ran(gpu, t == "i32") + [R.UNSUPPORTED]
        print(entry, width, t, names)
        assert names == plan
        # the next search on the same workspace is right
        out, cnt = _sync_search(gpu, "lattice", 0.75, 50, t)
        assert np.array_equal(_np(out), _want_rows("lattice", 0.75, 50)) and np.array_equal(_np(cnt), reference("lattice", 0.75)[1])
        out, _ = _sync_search(gpu, "clump2048", RADIUS, 0, t)
        assert np.array_equal(_np(out), _want_rows("clump2048", RADIUS, 2048))


def _grid_sections(grid):
    g, cs, e = R.parse_grid(_np(grid.blob), grid.nb, grid.cells, grid.ns)
    return g.tobytes(), cs.tobytes(), e.tobytes()


@pytest.mark.parametrize("name,r,width,wide", DEFERRED, ids=["%s-r%g-w%d-caps%d" % c for c in DEFERRED])
def test_deferred(gpu, name, r, width, wide):
    d = dataset(name)
    keys, counts = reference(name, r)
    mc, ns = int(counts.max()), len(d["s"])
    cap = R.async_cap(width, wide)
    plan = R.fill_plan("async", width, mc, wide)
    within = counts <= cap                                        # rows whose every neighbour fitted the slab of the first pass
    want_first, want_kl = R.rows(keys, counts, width, ns), R.key_last(keys, counts, width)
    qd, sd = _dev(gpu, name)
    got = []
    for _ in range(2):
        _set_wide_caps(wide)
        ds = ops.DeferredSearches(gpu)
        out, order, grid = ds.add(qd, sd, d["ql"], d["sl"], r, width, want_order=True, want_grid=True)
        names = ran(gpu, False, beside=True)
        assert grid.cap == cap and names == plan[:1]
        first, kl = _np(out), _np(grid.key_last).view(np.uint64)
        fin = ds.finish()
        assert ds.last_counts == [mc]
        if mc > cap:
            names += ran(gpu, False)
        print(name, r, width, wide, names)
        assert names == plan
        assert np.array_equal(first[within], want_first[within]) and np.array_equal(kl[within], want_kl[within])
        assert np.array_equal(_np(fin[0]), _want_rows(name, r, width))
        grids = R.check_grid(_np(grid.blob), grid.nb, grid.cells, grid.ns, _np(order), d["s"], d["sl"], r)
        if name == "line":                                        # the cell grew: at least one factor of 1.26 above 1.001 r
            assert np.float32(grids[0]["inv_cell"]) * np.float32(r) < 1 / 1.26
        got.append((first[within], kl[within], _np(fin[0]), _np(order)) + _grid_sections(grid))
    for a, b in zip(*got):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b


def _raw_async(gpu, name, r, width, t, nearest=False, key_last=False):
    """the asynchronous entries through the C ABI -> (rows, device word, key_last)"""
    lib = _lib.lib()
    d = dataset(name)
    qd, sd = _dev(gpu, name)
    ws = ops._ws.neighbors(gpu)
    out = torch.empty((qd.shape[0],) if nearest else (qd.shape[0], width), dtype=DT[t], device=gpu)
    word = torch.full((1,), -7, dtype=torch.int32, device=gpu)
    kl = torch.empty((qd.shape[0],), dtype=torch.int64, device=gpu) if key_last else None
    o32, o64 = (ptr(out), None) if t == "i32" else (None, ptr(out))
    hq, hs = C.c_void_p(d["ql"].ctypes.data), C.c_void_p(d["sl"].ctypes.data)
    with torch.cuda.device(gpu):
        if key_last:
            check(lib.ws_radius_neighbors_set_key_last(ws, ptr(kl)))
        if nearest:
            check(lib.ws_radius_neighbors_nearest_async(ws, ptr(qd), qd.shape[0], ptr(sd), sd.shape[0], hq, hs, len(d["ql"]),
                                                        float(np.float32(r)), o32, o64, ptr(word), current_stream()))
        else:
            check(lib.ws_radius_neighbors_search_async(ws, ptr(qd), qd.shape[0], ptr(sd), sd.shape[0], hq, hs, len(d["ql"]),
                                                       float(np.float32(r)), width, o32, o64, ptr(word), current_stream()))
    torch.cuda.synchronize()
    return _np(out), int(word.item()), (_np(kl).view(np.uint64) if key_last else None)


@pytest.mark.parametrize("t", list(DT))
@pytest.mark.parametrize("name,r,width,wide", ASYNC_RAW, ids=["%s-r%g-w%d-caps%d" % c for c in ASYNC_RAW])
def test_async_entry_rows(gpu, name, r, width, wide, t):
    keys, counts = reference(name, r)
    ns = len(dataset(name)["s"])
    cap = R.async_cap(width, wide)
    within = counts <= cap
    want, want_kl = R.rows(keys, counts, width, ns), R.key_last(keys, counts, width)
    got = []
    for _ in range(2):
        _set_wide_caps(wide)
        assert _lib.lib().ws_radius_neighbors_async_cap(width) == cap
        out, word, kl = _raw_async(gpu, name, r, width, t, key_last=True)
        names = ran(gpu, t == "i32", beside=True)
        print(name, r, width, wide, t, names)
        assert names == R.fill_plan("async", width, int(counts.max()), wide, t == "i32")[:1]
        assert word == int(counts.max())
        assert np.array_equal(out[within], want[within]) and np.array_equal(kl[within], want_kl[within])
        got.append((out[within], kl[within]))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


@pytest.mark.parametrize("t", list(DT))
def test_key_last_of_truncated_rows_on_the_2048_slab(gpu, t):
    """nb_fill_kernel<2048> is reached through the synchronous entries only (the asynchronous slabs end at 1024): a one-pass
    search at width 128 over rows of up to 1025 neighbours re-runs into the 2048 slab, and the key_last it leaves is the
    (distance, index) key of column 127 of every truncated row, all ones elsewhere"""
    name, r, width = "clump1025", RADIUS, 128
    keys, counts = reference(name, r)
    d = dataset(name)
    ns = len(d["s"])
    assert int(counts.max()) == 1025 and (counts > width).any() and (counts <= width).any()
    lib = _lib.lib()
    qd, sd = _dev(gpu, name)
    ws = ops._ws.neighbors(gpu)
    out = torch.empty((qd.shape[0], width), dtype=DT[t], device=gpu)
    kl = torch.empty((qd.shape[0],), dtype=torch.int64, device=gpu)
    o32, o64 = (ptr(out), None) if t == "i32" else (None, ptr(out))
    mc = C.c_int32(0)
    with torch.cuda.device(gpu):
        check(lib.ws_radius_neighbors_set_key_last(ws, ptr(kl)))
        check(lib.ws_radius_neighbors_search(ws, ptr(qd), qd.shape[0], ptr(sd), sd.shape[0], C.c_void_p(d["ql"].ctypes.data),
                                             C.c_void_p(d["sl"].ctypes.data), len(d["ql"]), float(np.float32(r)), width, o32, o64,
                                             C.byref(mc), current_stream()))
    torch.cuda.synchronize()
    names = ran(gpu, t == "i32")
    print(name, r, width, t, names)
    assert names == R.fill_plan("search", width, 1025, 1, t == "i32") and "nb_fill_kernel<2048," in names[-1]
    assert mc.value == 1025
    assert np.array_equal(_np(out), R.rows(keys, counts, width, ns))
    assert np.array_equal(_np(kl).view(np.uint64), R.key_last(keys, counts, width))


@pytest.mark.parametrize("t", list(DT))
@pytest.mark.parametrize("name,r", NEAREST, ids=["%s-r%g" % c for c in NEAREST])
def test_nearest(gpu, name, r, t):
    keys, counts = reference(name, r)
    ns = len(dataset(name)["s"])
    want = R.nearest(keys, counts, ns)
    got = []
    for _ in range(2):
        out, word, _ = _raw_async(gpu, name, r, 1, t, nearest=True)
        names = ran(gpu, t == "i32")
        print(name, r, t, names)
        assert names == R.fill_plan("nearest", 1, 0, 1, t == "i32")
        assert np.array_equal(out, want)
        assert word == (1 if counts.max() > 0 else 0)
        got.append(out)
    assert np.array_equal(got[0], got[1])
    if name == "nowhere":
        assert (want == ns).all()
    else:
        assert (want == ns).any() == bool((counts == 0).any())


@pytest.mark.parametrize("name,r,entry,width", CLONE, ids=["%s-r%g-%s-w%d" % c for c in CLONE])
def test_self_query_through_a_clone(gpu, name, r, entry, width):
    """queries with the supports' values behind another pointer: the queries are walked in index order, not in cell order"""
    d = dataset(name)
    assert d["self_query"]
    _, sd = _dev(gpu, name)
    want = _want_rows(name, r, width or max_count(name, r))
    for q in (sd, sd.clone()):
        for _ in range(2):
            if entry == "async":
                ds = ops.DeferredSearches(gpu)
                ds.add(q, sd, d["ql"], d["sl"], r, width)
                out = ds.finish()[0]
            else:
                out, _ = _sync_search(gpu, name, r, width, "i64", q=q)
            assert np.array_equal(_np(out), want)


def _deferred_rows(gpu, q, s, ql, sl, r, width, reuse):
    ds = ops.DeferredSearches(gpu)
    ds.add(q, s, ql, sl, r, width, reuse_grid=reuse)
    return _np(ds.finish()[0])


def _brute_rows(q, s, ql, sl, r, width):
    keys, counts = R.brute_keys(q, s, ql, sl, r)
    return R.rows(keys, counts, min(width, int(counts.max())), len(s))


def test_reuse_grid(gpu):
    """a second search over the same supports keeps the grid and equals a fresh one; anything checkable that differs (tensor,
    lengths, radius) makes the request fall back to a rebuild; the request is one-shot"""
    d, x = dataset("uniform"), dataset("uniform_x")
    qd, sd = _dev(gpu, "uniform_x")
    w = 40
    for _ in range(2):
        assert np.array_equal(_deferred_rows(gpu, sd, sd, d["ql"], d["sl"], 0.5, w, False), _want_rows("uniform", 0.5, w))
        assert np.array_equal(_deferred_rows(gpu, qd, sd, x["ql"], x["sl"], 0.5, w, True), _want_rows("uniform_x", 0.5, w))
        # one-shot: the next search, over other supports of the same shape, builds its own grid
        moved = (sd + 0.05).contiguous()
        assert np.array_equal(_deferred_rows(gpu, qd, moved, x["ql"], x["sl"], 0.5, w, False),
                              _brute_rows(x["q"], _np(moved), x["ql"], x["sl"], 0.5, w))
        # fall-backs, each after a search over (sd, lens, 0.5): another tensor, other lengths, another radius
        other_lens = np.array([600, 100, 500], np.int32)
        for s2, sl2, r2 in ((moved, x["sl"], 0.5), (sd, other_lens, 0.5), (sd, x["sl"], 0.4)):
            _deferred_rows(gpu, sd, sd, d["ql"], d["sl"], 0.5, w, False)
            assert np.array_equal(_deferred_rows(gpu, qd, s2, x["ql"], sl2, r2, w, True),
                                  _brute_rows(x["q"], _np(s2), x["ql"], sl2, r2, w))
    # 70 elements do not fit the argument table of the query update: rebuilt
    m, mx = dataset("many"), dataset("many_x")
    qm, sm = _dev(gpu, "many_x")
    assert np.array_equal(_deferred_rows(gpu, sm, sm, m["ql"], m["sl"], 0.5, 30, False), _want_rows("many", 0.5, 30))
    assert np.array_equal(_deferred_rows(gpu, qm, sm, mx["ql"], mx["sl"], 0.5, 30, True), _want_rows("many_x", 0.5, 30))


def test_reuse_request_is_consumed_by_one_search(gpu):
    """The kept grid holds its own copy of the supports (the caller vouches that they did not change).  Changing them in
    place shows which searches read the kept copy: the one that carries the request does, the one after it does not."""
    x = dataset("uniform_x")
    qd, _ = _dev(gpu, "uniform_x")
    s_old = dataset("uniform")["s"]
    sd = torch.from_numpy(s_old).to(gpu)
    w = 40
    d = dataset("uniform")
    assert np.array_equal(_deferred_rows(gpu, sd, sd, d["ql"], d["sl"], 0.5, w, False), _want_rows("uniform", 0.5, w))
    sd.add_(0.05)
    s_new = _np(sd)
    old, new = _want_rows("uniform_x", 0.5, w), _brute_rows(x["q"], s_new, x["ql"], x["sl"], 0.5, w)
    assert not np.array_equal(old, new)
    assert np.array_equal(_deferred_rows(gpu, qd, sd, x["ql"], x["sl"], 0.5, w, True), old)
    assert np.array_equal(_deferred_rows(gpu, qd, sd, x["ql"], x["sl"], 0.5, w, False), new)
