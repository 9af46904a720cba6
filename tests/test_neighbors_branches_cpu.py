"""CPU side of tests/test_neighbors_branches_gpu.py: the brute-force reference of oracle/neighbors_ref.py is right, its
restatement of the launcher's slab rules is the library's, the case tables reach every launch form and straddle every step,
the data sets hold what the cases rely on, and the comparison the GPU tests use rejects small mutations of a right result.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import test_neighbors_branches_gpu as NB
from conftest import assert_neighbors_equal, golden
from oracle import geom
from oracle import neighbors_ref as R
from weasal_amd import _lib

SET_RADII = sorted({(c[0], c[1]) for c in NB.PLAN_FILL + NB.SEARCH + NB.DEFERRED + NB.ASYNC_RAW + NB.NEAREST + NB.CLONE}
                   | {("clump2049", 0.5)})


# ------------------------------------------------------------------------------------------------------------------
# the reference is right
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,r", SET_RADII, ids=["%s-r%g" % c for c in SET_RADII])
def test_brute_keys_equal_the_cpu_oracles(name, r):
    d = NB.dataset(name)
    keys, counts = NB.reference(name, r)
    ns = len(d["s"])
    assert keys.dtype == np.uint64 and np.all(np.diff(keys.astype(np.float64), axis=1) >= 0)
    for row, c in zip(keys[::97], counts[::97]):
        assert np.all(row[:c] != R.ALL_ONES) and np.all(row[c:] == R.ALL_ONES) and np.all(np.diff(row[:c].astype(object)) > 0)
    if counts.max() == 0:
        with pytest.raises(RuntimeError):
            geom.batch_query(d["q"], d["s"], d["ql"], d["sl"], r, kind="port")
        return
    want = R.rows(keys, counts, int(counts.max()), ns)
    port = geom.batch_query(d["q"], d["s"], d["ql"], d["sl"], r, kind="port")
    assert np.array_equal(want, port.astype(np.int64))
    # the reference steps to the next element once per query (neighbors.cpp:272-276), so an element without queries
    # leaves it one element behind: its answer is meaningful only where every element has queries and supports
    if geom.have_ref() and d["ql"].min() > 0 and d["sl"].min() > 0:
        ref = geom.batch_query(d["q"], d["s"], d["ql"], d["sl"], r, kind="ref")
        assert_neighbors_equal(d["q"], d["s"], ref.astype(np.int64), want, False)


def test_brute_keys_agree_with_g1():
    g = golden("g1_neighbors.npz")
    p, l, sp, sl = g["points"], g["lens"], g["sub_points"], g["sub_lens"]
    for r in (0.6, 1.0):
        for tag, q, ql, s, ssl, rr in (("self", p, l, p, l, r), ("pool", sp, sl, p, l, r), ("up", p, l, sp, sl, 2 * r)):
            keys, counts = R.brute_keys(q, s, ql, ssl, rr)
            got = R.rows(keys, counts, int(counts.max()), len(s))
            assert_neighbors_equal(q, s, got, g["%s_r%.1f" % (tag, rr)].astype(np.int64), bool(g["tiefree_%s_r%.1f" % (tag, rr)]))


def test_helpers_on_a_hand_made_case():
    s = np.array([[0, 0, 0], [0.3, 0, 0], [-0.3, 0, 0], [0.5, 0, 0], [9, 9, 9]], np.float32)
    q = np.array([[0, 0, 0], [5, 5, 5]], np.float32)
    keys, counts = R.brute_keys(q, s, [2], [5], 0.5)
    assert counts.tolist() == [3, 0] and keys.shape == (2, 3)
    assert R.rows(keys, counts, 4, 5).tolist() == [[0, 1, 2, 5], [5, 5, 5, 5]]           # the tie 1 / 2 falls to the index
    assert R.rows(keys, counts, 2, 5).tolist() == [[0, 1], [5, 5]]
    assert R.nearest(keys, counts, 5).tolist() == [0, 5]
    d2 = np.float32(0.3) * np.float32(0.3)
    assert R.key_last(keys, counts, 2).tolist() == [(int(d2.view(np.uint32)) << 32) | 1, int(R.ALL_ONES)]
    assert R.key_last(keys, counts, 3).tolist() == R.key_last(keys, counts, 9).tolist() == [int(R.ALL_ONES)] * 2
    # elements do not see each other
    keys, counts = R.brute_keys(q[:1], s, [0, 1], [4, 1], 0.5)
    assert counts.tolist() == [0]
    # chunking does not change anything
    d = NB.dataset("uniform_x")
    a = R.brute_keys(d["q"], d["s"], d["ql"], d["sl"], 0.5)
    b = R.brute_keys(d["q"], d["s"], d["ql"], d["sl"], 0.5, chunk_pairs=1000)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------------------------
# the plan mirror is the library's
# ------------------------------------------------------------------------------------------------------------------
def _variant(cap, i32, beside):
    lib = _lib.lib()
    buf = C.create_string_buffer(96)
    rc = lib.ws_radius_neighbors_fill_variant(cap, i32, beside, buf, 96)
    if rc == 2:
        assert b"exceeds the 2048-entry sort slab" in lib.ws_last_error()
        return R.UNSUPPORTED
    assert rc == 0
    return buf.value.decode()


def test_fill_names_are_the_reporters():
    for cap, i32, beside in itertools.product(range(0, 2101), (0, 1), (0, 1)):
        assert R.fill_name(cap, bool(i32), bool(beside)) == _variant(cap, i32, beside), (cap, i32, beside)
    assert _lib.lib().ws_radius_neighbors_fill_variant(-1, 0, 0, C.create_string_buffer(8), 8) == 1
    assert _variant(704, 0, 1) == "nb_fill_wide_kernel<int64,704> grid<=1024"
    assert R.fill_plan("search", 128, 1025, out_i32=True) == ["nb_fill128_kernel<int32> grid<=4096", "nb_fill_kernel<2048,int32> grid<=4096"]
    assert R.fill_plan("async", 461, 577) == ["nb_fill_wide_kernel<int64,576> grid<=1024", "nb_fill_wide_kernel<int64,1024> grid<=4096"]
    assert R.fill_plan("plan_fill", 0, 2049) == [R.UNSUPPORTED] and R.fill_plan("plan_fill", 0, 0) == []


def test_async_cap_is_the_librarys():
    lib = _lib.lib()
    flag = C.c_int.in_dll(lib, "ws_nb_wide_caps")
    saved = flag.value
    try:
        for wide in (1, 0):
            flag.value = wide
            for w in range(1, 1301):
                assert lib.ws_radius_neighbors_async_cap(w) == R.async_cap(w, wide), (w, wide)
    finally:
        flag.value = saved
    # the steps of the rule, computed from it: need = w + w // 4 against 576 and 704
    steps = [w for w in range(1, 1300) if R.async_cap(w) != R.async_cap(w + 1)]
    assert steps == [128, 461, 563]


def test_last_fills_needs_no_search():
    lib = _lib.lib()
    ws = C.c_void_p()
    assert lib.ws_neighbors_ws_create(C.byref(ws)) == 0
    n = C.c_int32(-1)
    assert lib.ws_radius_neighbors_last_fills(ws, None, 0, C.byref(n)) == 0 and n.value == 0
    assert lib.ws_radius_neighbors_last_fills(None, None, 0, C.byref(n)) == 1
    lib.ws_neighbors_ws_destroy(ws)


# ------------------------------------------------------------------------------------------------------------------
# the case tables cover the ladders
# ------------------------------------------------------------------------------------------------------------------
SWEEP_WIDTHS = (1, 100, 128, 129, 300, 461, 462, 563, 564, 1024, 1300, 2100)
SWEEP_COUNTS = (0, 1, 128, 129, 576, 577, 704, 705, 1024, 1025, 2048, 2049, 3000)


def sweep_names():
    names = set()
    for entry, w, mc, wide, i32 in itertools.product(R.ENTRIES, SWEEP_WIDTHS, SWEEP_COUNTS, (1, 0), (False, True)):
        names.update(R.fill_plan(entry, w, mc, wide, i32))
    return names


def test_case_tables_cover_every_plan_name():
    swept = sweep_names()
    table = set()
    for _entry, _t, plan in NB.case_plans():
        table.update(plan)
    print("launch forms reached by the GPU case tables: %d / %d" % (len(swept & table), len(swept)))
    for p in sorted(table):
        print("  " + p)
    assert table == swept, (sorted(swept - table), sorted(table - swept))
    # counted: five slabs on the synchronous grid, four beside a training stream, the nearest-only kernel, each for both
    # row types, and the refusal
    assert len(swept) == 2 * (5 + 4 + 1) + 1


def test_tables_straddle_every_step():
    plans = NB.case_plans()
    mc = lambda name, r: NB.max_count(name, r)
    # row counts on either side of every slab step, through plan + fill (cap = count) ...
    pf = {mc(n, r) for n, r in NB.PLAN_FILL}
    assert {128, 129, 576, 577, 704, 705, 1024, 1025, 2048} <= pf and ("plan_fill", 0) in NB.UNSUPPORTED
    # ... and through the re-run of the synchronous search, narrow and wide
    narrow = {mc(n, r) for n, r, w, _ in NB.SEARCH if w <= 128}
    assert {128, 129, 576, 577, 704, 705, 1024, 1025, 2048} <= narrow and ("search", 128) in NB.UNSUPPORTED
    wide = {mc(n, r) for n, r, w, _ in NB.SEARCH if w > 128}
    assert {128, 1024, 1025, 2048} <= wide and any(w > 128 for e, w in NB.UNSUPPORTED if e == "search")
    # widths against the count: 1, below, equal, above
    for name, r in (("lattice", 0.75), ("clump2048", 0.5)):
        ws = {w for n, rr, w, _ in NB.SEARCH if (n, rr) == (name, r)}
        m = mc(name, r)
        assert 1 in ws and m in ws and any(w > m for w in ws) and (name != "lattice" or any(1 < w < m for w in ws))
    # asynchronous widths on either side of every step of the rule, each slab with and without overflow
    widths = {w for _, _, w, wide in NB.DEFERRED if wide}
    assert {128, 129, 461, 462, 563, 564} <= widths
    seen = {(R.async_cap(w, wide), mc(n, r) > R.async_cap(w, wide)) for n, r, w, wide in NB.DEFERRED}
    assert seen == set(itertools.product((128, 576, 704, 1024), (False, True)))
    edge = {(R.async_cap(w, wide), mc(n, r) - R.async_cap(w, wide)) for n, r, w, wide in NB.DEFERRED}
    assert {(c, d) for c in (128, 576, 704, 1024) for d in (0, 1)} <= edge          # a full slab, and one neighbour too many
    assert any(not wide and w > 128 for _, _, w, wide in NB.DEFERRED)
    assert {p[0] for _, _, p in plans if p} >= {R.fill_name(c, i, True) for c in (128, 576, 704, 1024) for i in (False, True)}
    # truncated rows carry a real key_last on every slab of the asynchronous pass
    assert {R.async_cap(w, wide) for n, r, w, wide in NB.DEFERRED if w < mc(n, r) <= R.async_cap(w, wide)} == {128, 576, 704, 1024}
    # the grids: past the synchronous 4096-workgroup cap, past the asynchronous 1024, and the small roundings
    assert any(len(NB.dataset(n)["q"]) > 4 * 4096 for n, _ in NB.PLAN_FILL) and any(len(NB.dataset(n)["q"]) > 4 * 4096 for n, *_ in NB.SEARCH)
    assert any(len(NB.dataset(n)["q"]) > 4 * 1024 for n, *_ in NB.DEFERRED)
    assert {len(NB.dataset(n)["q"]) for n, *_ in NB.SEARCH} >= set(NB.TINY_NQ)


# ------------------------------------------------------------------------------------------------------------------
# the data holds what the cases rely on
# ------------------------------------------------------------------------------------------------------------------
def _d2(keys):
    return (keys >> np.uint64(32)).astype(np.uint32)


def test_clump_rows_have_exactly_the_intended_count():
    for m in NB.CLUMP_M:
        d = NB.dataset("clump%d" % m)
        _, counts = NB.reference("clump%d" % m)
        assert d["in_clump"].sum() == m and np.all(counts[d["in_clump"]] == m)
        assert counts[~d["in_clump"]].max() < 64 and counts.max() == m
        assert len(d["s"]) == NB.SCATTER_N + m


def test_lattice_rows_ties_and_the_excluded_radius():
    d = NB.dataset("lattice")
    for r, rows in NB.LATTICE_ROWS.items():
        keys, counts = NB.reference("lattice", r)
        assert counts.max() == rows
        mid = int(np.argmin(np.abs(d["q"] - np.float32((NB.LATTICE_N // 2) * NB.LATTICE_STEP)).sum(1)))      # the centre point
        assert counts[mid] == rows
        full = keys[mid]
        _, mult = np.unique(_d2(full[:rows]), return_counts=True)
        assert mult.max() >= (20 if r >= 0.75 else 6) and (rows - len(mult)) >= 20          # exact d2 ties in one row
        # d = r occurs exactly and is excluded: the full row misses the 6 axis neighbours at distance r
        centre = d["q"][mid].astype(np.float64)
        dist2 = ((d["s"].astype(np.float64) - centre) ** 2).sum(1)
        assert (dist2 == r * r).sum() >= 6 and (dist2 < r * r).sum() == rows
    keys, counts = NB.reference("lattice_mid", 0.5)
    assert np.all(counts >= 8) and np.all(_d2(keys[:, :8]) == _d2(keys[:, :1]))              # eight nearest, all tied


def test_coincident_sets_fill_one_bucket():
    for n, slab in ((600, 704), (100, 128)):
        d = NB.dataset("coincident%d" % n)
        keys, counts = NB.reference("coincident%d" % n)
        first = int(np.nonzero(d["copies"])[0][0])
        row = keys[first]
        assert (_d2(row) == 0).sum() == n and n < counts.max() <= slab
        # the kernels' buckets, min(NB - 1, (int)(d2 * (NB / r^2))) with NB = 256 (wide) / 64 (128 slab): one of them holds
        # more keys than a wave has lanes (600: more than there are buckets), so the within-bucket loop runs that long
        nbuckets = 256 if slab > 128 else 64
        d2 = _d2(row[:counts[first]]).view(np.float32)
        bucket = np.minimum(nbuckets - 1, (d2 * (np.float32(nbuckets) / np.float32(0.25))).astype(np.int64))
        assert np.bincount(bucket).max() >= n > (256 if n == 600 else 64)


def test_near_radius_pairs():
    d = NB.dataset("near")
    keys, counts = NB.reference("near")
    q, s = d["q"].astype(np.float64), d["s"].astype(np.float64)
    inside = excluded = 0
    q0 = s0 = 0
    for nq, ns in zip(d["ql"], d["sl"]):
        dist = np.sqrt(((q[q0:q0 + nq, None, :] - s[None, s0:s0 + ns, :]) ** 2).sum(2))      # exact: one axis, representable
        inside += (np.abs(dist - (0.5 - NB.NEAR_EPS)) == 0).sum()
        excluded += ((dist == 0.5) | (dist == 0.5 + NB.NEAR_EPS)).sum()
        q0, s0 = q0 + nq, s0 + ns
    assert (inside, excluded) == (858, 1287) and inside >= 800 and excluded >= 1200
    assert counts.sum() == inside and counts.max() == 1 and (counts == 0).sum() == excluded
    # about 500 cells along each axis, no growth
    for b in range(3):
        sb = d["s"][b * NB.NEAR_K:(b + 1) * NB.NEAR_K]
        steps, dims = R.grid_dims(sb.min(0), sb.max(0), 0.5, NB.NEAR_K)
        assert steps == 0 and max(dims) > 490 and sorted(dims)[:2] == [1, 1]


def test_empty_rows_elements_and_far_queries():
    for name in ("uniform_x", "long_q", "near", "degenerate"):
        assert (NB.reference(name, 0.4 if name == "long_q" else 0.5)[1] == 0).any(), name
    u = NB.dataset("uniform")
    assert u["sl"].tolist() == [700, 0, 500] and u["ql"][1] == 0                  # an empty element in the middle
    d = NB.dataset("degenerate")
    pairs = list(zip(d["ql"].tolist(), d["sl"].tolist()))
    assert any(q == 0 and s > 0 for q, s in pairs) and any(q > 0 and s == 0 for q, s in pairs) and (0, 0) in pairs[1:-1]
    assert 1 in d["sl"] and 2 in d["sl"]
    # the last element: coplanar supports, queries more than two cells outside their box on every side
    ns, nq = int(d["sl"][-1]), int(d["ql"][-1])
    sb, qb = d["s"][-ns:], d["q"][-nq:]
    assert np.ptp(sb[:, 2]) == 0 and np.ptp(sb[:, 0]) > 3
    cell = 0.5 * 1.001
    below = ((sb.min(0) - qb) > 2 * cell).any(1)
    above = ((qb - sb.max(0)) > 2 * cell).any(1)
    assert below.sum() >= 3 and above.sum() >= 4 and (below | above).sum() == d["far"]
    assert (np.abs(qb) >= 3e5).any()                                              # far enough for the clamp of cell_coord
    _, counts = NB.reference("degenerate")
    assert np.all(counts[-nq:][below | above] == 0)
    assert len(NB.dataset("many")["sl"]) == 70 and NB.dataset("many")["sl"].min() >= 20 and NB.dataset("many")["sl"].max() <= 60
    off = NB.dataset("offset")["s"]
    assert np.abs(off.mean(0) - (1001, 2000, 50)).max() < 2


def test_line_forces_cell_growth():
    d = NB.dataset("line")
    s = d["s"]
    assert len(s) == NB.LINE_N and np.ptp(s[:, 0]) >= NB.LINE_LENGTH
    # at the first cell, 1.001 r, the x dimension alone exceeds both limits of nb_grid_setup_kernel
    first = int(np.floor(np.float32(np.ptp(s[:, 0])) / (np.float32(0.5) * np.float32(1.001)))) + 1
    assert first > R.MAX_DIM and first > R.cell_cap(len(s))
    steps, dims = R.grid_dims(s.min(0), s.max(0), 0.5, len(s))
    assert steps >= 1 and max(dims) <= R.MAX_DIM and np.prod(dims) <= R.cell_cap(len(s))
    _, counts = NB.reference("line")
    assert counts.max() >= 2


def test_check_grid_accepts_a_hand_built_grid_and_rejects_a_misfiled_entry():
    """check_grid on a grid built here with the setup rule, then on small corruptions of it"""
    d = NB.dataset("degenerate")
    s, sl, r = d["s"], d["sl"], 0.5
    nb, ns = len(sl), len(s)
    cells = sum(R.cell_cap(n) for n in sl)
    grids = np.zeros(nb, R.CLOUD_GRID)
    cell_of = np.zeros(ns, np.int64)
    s0 = c0 = 0
    for b, n in enumerate(sl):
        g = grids[b]
        g["s_base"], g["s_len"], g["cell_base"], g["cell_cap"] = s0, n, c0, R.cell_cap(n)
        g["nx"] = g["ny"] = g["nz"] = 1
        g["inv_cell"] = 1
        if n:
            sb = s[s0:s0 + n]
            steps, dims = R.grid_dims(sb.min(0), sb.max(0), r, n)
            inv = np.float32(1) / (np.float32(r) * np.float32(1.001) * np.float32(1.26) ** steps)
            g["lo"], g["inv_cell"], (g["nx"], g["ny"], g["nz"]) = sb.min(0), inv, dims
            c = [np.clip(R.cell_coord(sb[:, k], sb[:, k].min(), inv), 0, dims[k] - 1) for k in range(3)]
            cell_of[s0:s0 + n] = c0 + (c[2] * dims[1] + c[1]) * dims[0] + c[0]
        s0, c0 = s0 + n, c0 + R.cell_cap(n)
    order = np.lexsort((np.arange(ns), cell_of))
    cell_start = np.zeros(cells + 2, np.int32)
    cell_start[1:cells + 1] = np.cumsum(np.bincount(cell_of, minlength=cells))
    entries = np.zeros((ns, 4), np.float32)
    entries[:, :3] = s[order]
    entries[:, 3] = order.astype(np.int32).view(np.float32)

    def blob(gr=grids, cs=cell_start, en=entries):
        c_off = R._align(nb * R.CLOUD_GRID.itemsize)
        s_off = c_off + R._align((cells + 2) * 4)
        out = np.zeros(s_off + 16 * ns, np.uint8)
        out[:gr.nbytes] = gr.view(np.uint8)
        out[c_off:c_off + cs.nbytes] = cs.view(np.uint8)
        out[s_off:] = en.view(np.uint8).reshape(-1)
        return out

    R.check_grid(blob(), nb, cells, ns, order, s, sl, r)
    swapped = entries.copy()
    a = int(np.nonzero(np.diff(cell_of[order]) > 0)[0][0])          # two neighbours of different cells trade places
    swapped[[a, a + 1]] = swapped[[a + 1, a]]
    descending = entries.copy()
    a = int(np.nonzero(np.diff(cell_of[order]) == 0)[0][0])         # two entries of one cell in descending index order
    descending[[a, a + 1]] = descending[[a + 1, a]]
    moved = entries.copy()
    moved[5, 0] = np.nextafter(moved[5, 0], np.float32(9))
    tight = grids.copy()
    tight["inv_cell"][-1] = np.float32(2.0)                         # cell == radius: no margin
    short = cell_start.copy()
    short[1] += 1
    for bad in (dict(en=swapped), dict(en=descending), dict(en=moved), dict(gr=tight), dict(cs=short)):
        with pytest.raises(AssertionError):
            R.check_grid(blob(**bad), nb, cells, ns, None, s, sl, r)
    with pytest.raises(AssertionError):
        R.check_grid(blob(), nb, cells, ns, order[::-1], s, sl, r)


# ------------------------------------------------------------------------------------------------------------------
# teeth: what the GPU tests compare with (np.array_equal against rows / key_last of the reference) rejects near misses
# ------------------------------------------------------------------------------------------------------------------
def test_the_comparison_rejects_small_mutations():
    d = NB.dataset("lattice")
    ns = len(d["s"])
    keys, counts = NB.reference("lattice", 0.75)
    want = R.rows(keys, counts, 93, ns)
    q = int(np.argmax(counts))
    row = keys[q]
    tie = int(np.nonzero(_d2(row[1:93]) == _d2(row[:92]))[0][0])
    swapped = want.copy()
    swapped[q, [tie, tie + 1]] = swapped[q, [tie + 1, tie]]
    assert not np.array_equal(swapped, want)
    assert_neighbors_equal(d["q"], d["s"], swapped, want, False)        # ... which the tie-tolerant comparison lets through
    # the entry just inside the radius dropped / the entry at exactly r added (the near-radius set: rows of one or none)
    n = NB.dataset("near")
    nk, nc = NB.reference("near")
    nwant = R.rows(nk, nc, 1, len(n["s"]))
    inside = int(np.nonzero(nc == 1)[0][0])
    dropped = nwant.copy()
    dropped[inside, 0] = len(n["s"])
    assert not np.array_equal(dropped, nwant)
    dist = np.abs(n["q"][:, None, :].astype(np.float64) - n["s"][None, :, :].astype(np.float64)).sum(2)
    at_r = np.argwhere(dist == 0.5)
    at_r = [(a, b) for a, b in at_r if nc[a] == 0 and _same_element(n, a, b)][0]
    added = nwant.copy()
    added[at_r[0], 0] = at_r[1]
    assert not np.array_equal(added, nwant)
    k_incl, c_incl = R.brute_keys(n["q"], n["s"], n["ql"], n["sl"], np.nextafter(np.float32(0.5), np.float32(1)))
    assert c_incl[at_r[0]] == 1 and not np.array_equal(R.rows(k_incl, c_incl, 1, len(n["s"])), nwant)   # "<=" instead of "<"
    # padding with ns - 1
    padded = np.where(want == ns, ns - 1, want)
    assert (want == ns).any() and not np.array_equal(padded, want)
    # key_last one position off
    kl = R.key_last(keys, counts, 50)
    assert (counts > 50).any() and (kl[counts <= 50] == R.ALL_ONES).all()
    for off in (49 - 1, 49 + 1):
        wrong = np.where(counts > 50, keys[:, off], R.ALL_ONES)
        assert not np.array_equal(wrong, kl)
    assert not np.array_equal(R.key_last(keys, counts, 51), kl)


def _same_element(d, qi, si):
    qe = np.searchsorted(np.cumsum(d["ql"]), qi, side="right")
    se = np.searchsorted(np.cumsum(d["sl"]), si, side="right")
    return qe == se
