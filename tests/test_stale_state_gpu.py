"""GPU: the state that CHOOSES a kernel path or a slab, not the kernels themselves.

Two kinds of process state decide what a call does without being part of its arguments:

  * the sort slab of the asynchronous radius search (ws_radius_neighbors_async_cap: 576 / 704 / 1024 keys per query),
    which depends on the process-global `ws_nb_wide_caps`; ops.widen_async_slabs sets it to 0 (1024 keys) as soon as one
    search overflows.  The validity of a search must be judged against the slab it was LAUNCHED with, not against the
    global after the synchronisation: a 576-key row with 577..1024 neighbours holds an arbitrary subset of them.
  * the index hints of ops (distance-sorted rows, search grids, transposed tables, pooling orders), looked up by the
    address of an index matrix.  A hint must answer only for the tensor it was registered with, at the version it had:
    a matrix at a recycled address, or one changed in place, would otherwise be walked as if it were the old one.

Every result is compared with the CPU oracle (oracle/geom.py = the reference's compiled core when oracle/_ref is present,
oracle/pyramid_ref.py, oracle/kpconv_ref.py in float64).
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import assert_neighbors_equal, sphere

pytestmark = pytest.mark.gpu

LIMITS = [422, 519, 472, 193, 34]       # the config-5 workload's limits: slab 576 at level 0 (422 + 422 / 4 = 527)
R_DENSE = 2.0                           # level-0 search radius of the deformable config (0.4 * 2.5 * 5.0 / 2.5)


def _kind():
    from oracle import geom
    return "ref" if geom.have_ref() else "port"


def _caps_flag():
    from weasal_amd import _lib
    return C.c_int.in_dll(_lib.lib(), "ws_nb_wide_caps")


def _slab(width):
    from weasal_amd import _lib
    return int(_lib.lib().ws_radius_neighbors_async_cap(int(width)))


@pytest.fixture(autouse=True)
def _isolated():
    """every test leaves the slab switch and the hint registries as it found them"""
    from weasal_amd import ops
    flag = _caps_flag()
    saved = flag.value
    yield
    flag.value = saved
    ops.clear_batch_hints()
    ops.clear_point_orders()


def rel(a, ref):
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    return ((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def _dense_cloud():
    """one sphere of ~19 points / m^3: rows of the 2 m search hold up to ~710 neighbours, beyond the 576-key slab of limit
    422 and within the 1024-key one"""
    rng = np.random.default_rng(3)
    pts = sphere(rng, 6000, 4.2)
    return pts, np.array([6000], np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# launch-time slabs
# ---------------------------------------------------------------------------------------------------------------------
def test_two_overflowing_searches_in_one_finish(gpu):
    """two searches of one DeferredSearches both overflow their 576-key slab: the first one's overflow widens the process
    to 1024 keys inside finish(); the second must still be judged against the 576 keys it ran with and be redone"""
    from oracle import geom
    from weasal_amd import ops
    pts, lens = _dense_cloud()
    sub = pts[::3]
    sl = np.array([sub.shape[0]], np.int32)
    want_self = geom.batch_query(pts, pts, lens, lens, R_DENSE, kind=_kind())
    want_sub = geom.batch_query(sub, pts, sl, lens, R_DENSE, kind=_kind())
    _caps_flag().value = 1
    assert _slab(LIMITS[0]) == 576
    assert 576 < want_self.shape[1] <= 1024 and 576 < want_sub.shape[1] <= 1024      # both overflow the launch slab
    P = torch.from_numpy(pts).to(gpu)
    S = torch.from_numpy(sub).to(gpu)
    d = ops.DeferredSearches(gpu)
    d.add(P, P, lens, lens, R_DENSE, LIMITS[0])
    d.add(S, P, sl, lens, R_DENSE, LIMITS[0])
    fin = d.finish()
    assert d.last_counts == [want_self.shape[1], want_sub.shape[1]]
    assert_neighbors_equal(pts, pts, fin[0].cpu().numpy(), want_self[:, :LIMITS[0]].astype(np.int64), False)
    assert_neighbors_equal(sub, pts, fin[1].cpu().numpy(), want_sub[:, :LIMITS[0]].astype(np.int64), False)


def test_widening_between_add_and_finish(gpu):
    """another search of the process widens the slabs after this one was launched with 576 keys: finish() must redo the
    overflowed search, and its grid keeps the slab of the launch (key_last is valid up to it, no further)"""
    from oracle import geom
    from weasal_amd import ops
    pts, lens = _dense_cloud()
    want = geom.batch_query(pts, pts, lens, lens, R_DENSE, kind=_kind())
    _caps_flag().value = 1
    assert 576 < want.shape[1] <= 1024
    P = torch.from_numpy(pts).to(gpu)
    d = ops.DeferredSearches(gpu)
    _, _, grid = d.add(P, P, lens, lens, R_DENSE, LIMITS[0], want_order=True, want_grid=True)
    assert grid.cap == 576
    ops.widen_async_slabs(want.shape[1])
    assert _slab(LIMITS[0]) == 1024
    fin = d.finish()
    assert d.last_counts == [want.shape[1]]
    assert_neighbors_equal(pts, pts, fin[0].cpu().numpy(), want[:, :LIMITS[0]].astype(np.int64), False)
    assert grid.cap == 576
    # what pyramid.segmentation_inputs keeps a grid for (0 < max_count <= cap): not this search's
    assert not (0 < d.last_counts[0] <= grid.cap)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("native", [True, False], ids=["one_call", "per_call"])
def test_pyramid_judges_searches_by_their_launch_slab(gpu, native, monkeypatch):
    """the config-5 pyramid of a sphere dense enough that level 0 overflows its 576-key slab: every matrix against
    oracle.pyramid_ref, no grid for an overflowed search, and every grid's cap is the slab its search ran with.  One-call
    form: the descriptor records that slab per search, and a widening by another worker right after ws_pyramid_build
    returned (simulated by the wrapper below) changes nothing"""
    from oracle import geom, pyramid_ref
    from weasal_amd import _lib, config as wcfg, ops, pyramid
    cfg = wcfg.DALESDeformF32Config()
    pts, lens = _dense_cloud()
    n0 = pts.shape[0]
    feats = np.ones((n0, 3), np.float32)
    labels = np.zeros(n0, np.int64)
    r0 = cfg.first_subsampling_dl * cfg.deform_radius
    assert abs(r0 - R_DENSE) < 1e-12
    widest0 = geom.batch_query(pts, pts, lens, lens, r0, kind=_kind()).shape[1]
    _caps_flag().value = 1
    assert widest0 > _slab(LIMITS[0]) == 576                 # level 0 overflows the slab of its launch
    lib = _lib.lib()
    descs = []
    real_build = lib.ws_pyramid_build

    def build_then_widen(nws, sws, desc, stream):
        rc = real_build(nws, sws, desc, stream)
        if rc == 0:
            descs.append(desc._obj)
            _caps_flag().value = 0                           # another worker widened the slabs meanwhile
        return rc

    monkeypatch.setattr(pyramid, "NATIVE_PYRAMID", native)
    if native:
        monkeypatch.setattr(lib, "ws_pyramid_build", build_then_widen)
    np.random.seed(23)
    batch = pyramid.build_batch(cfg, torch.from_numpy(pts).to(gpu), torch.from_numpy(feats).to(gpu),
                                torch.from_numpy(labels).to(gpu), lens, LIMITS)
    np.random.seed(23)
    li = pyramid_ref.segmentation_inputs(cfg, pts, feats, labels, lens, LIMITS, kind=_kind())
    L = cfg.num_layers
    for l in range(L):
        p_l = li[l]
        assert np.array_equal(batch.points[l].cpu().numpy(), p_l), l
        assert_neighbors_equal(p_l, p_l, batch.neighbors[l].cpu().numpy(), li[L + l], False)
        if l < L - 1:
            nxt = li[l + 1]
            assert_neighbors_equal(nxt, p_l, batch.pools[l].cpu().numpy(), li[2 * L + l], False)
            assert_neighbors_equal(p_l, nxt, batch.upsamples[l].cpu().numpy(), li[3 * L + l], False)
    level_of = {id(m): l for l, m in enumerate(batch.neighbors)}
    grid_levels = [level_of[id(m)] for m, _ in batch.search_grids]
    assert 0 not in grid_levels and len(grid_levels) >= 2     # the overflowed search was redone: its grid is not used
    _caps_flag().value = 1
    for (m, grid), l in zip(batch.search_grids, grid_levels):
        assert grid.cap == _slab(LIMITS[l]), (l, grid.cap)
        assert 0 < grid.max_count <= grid.cap
    if native:
        d = descs[-1]
        for i in range(3 * L):
            w = int(d.width[i])
            assert int(d.cap[i]) == (_slab(w) if w > 0 else 0), (i, w, int(d.cap[i]))
        assert int(d.cap[0]) == 576 and int(d.max_count[0]) == widest0 and int(d.final_width[0]) == 0
        for (_, grid), l in zip(batch.search_grids, grid_levels):
            assert grid.cap == int(d.cap[3 * l])


# ---------------------------------------------------------------------------------------------------------------------
# index hints bound to their tensor
# ---------------------------------------------------------------------------------------------------------------------
RC, EXT, CI, CO = 1.0, 0.4, 16, 32      # KPConv radius / extent; the rows are searched with 2 RC (the deformable radius)


def _sorted_scene(gpu):
    rng = np.random.default_rng(21)
    pts = rng.uniform(-3, 3, size=(1200, 3)).astype(np.float32)
    P = torch.from_numpy(pts).to(gpu)
    lens = np.array([1200], np.int32)
    from weasal_amd import ops
    return P, ops.radius_neighbors(P, P, lens, lens, 2 * RC, dtype=torch.int64)      # rows sorted by distance, padded with n


def _stale_matrix(gpu, how):
    """a distance-sorted matrix M registered as sorted rows, then `how`:
    'recycled' -- M dropped, a new matrix U with the same neighbour sets in shuffled column order at M's address;
    'in_place' -- M's columns shuffled in place (same object, same address, bumped _version).  -> (points, U)"""
    from weasal_amd import ops
    P, M0 = _sorted_scene(gpu)
    n, h = M0.shape
    assert h > 100
    g = torch.Generator().manual_seed(5)
    perm = torch.argsort(torch.rand(n, h, generator=g), dim=1)
    shuffled = torch.gather(M0.cpu(), 1, perm).to(gpu)
    pool = torch.cuda.MemPool()             # a private pool: the next same-size request gets the freed block back
    with torch.cuda.use_mem_pool(pool):
        M = torch.empty_like(M0)
    M.copy_(M0)
    ops.active_hints().add(M, radius=2 * RC)
    assert ops.rows_cutoff_pays(M, RC)       # the hint applies to M itself
    addr, version = M.data_ptr(), M._version
    if how == "recycled":
        del M
        with torch.cuda.use_mem_pool(pool):
            U = torch.empty((n, h), dtype=torch.int64, device=gpu)
        assert U.data_ptr() == addr          # precondition: the address of the registered matrix is recycled
        U.copy_(shuffled)
    else:
        U = M
        U.copy_(shuffled)
        assert U.data_ptr() == addr and U._version != version
    U._pool = pool                          # (keeps the pool alive as long as U)
    return P, U


def _kpconv_vs_oracle(gpu, P, U, deformable):
    """blocks.KPConv (rigid linear, or deformable + modulated) forward, dX and dW on the GPU against its float64 CPU twin"""
    from oracle import kpconv_ref
    from weasal_amd.blocks import KPConv
    np.random.seed(1)
    torch.manual_seed(1)
    conv = KPConv(15, 3, CI, CO, EXT, RC, deformable=deformable, modulated=deformable)
    twin = copy.deepcopy(conv).double()
    conv = conv.to(gpu)
    n = P.shape[0]
    x = torch.randn(n, CI)
    dy = torch.randn(n, CO)
    xg = x.to(gpu).requires_grad_(True)
    out = conv(P, P, U, xg)
    (out * dy.to(gpu)).sum().backward()
    torch.cuda.synchronize()
    xc = x.double().requires_grad_(True)
    Pc = P.cpu().double()
    with kpconv_ref.cpu_reference_mode():
        ref = twin(Pc, Pc, U.cpu(), xc)
    (ref * dy.double()).sum().backward()
    return {"out": rel(out, ref), "dx": rel(xg.grad, xc.grad), "dW": rel(conv.weights.grad, twin.weights.grad)}


def _assert_bars(errs, deformable):
    if deformable:      # f32 bars of tests/test_config5_wide_gpu.py (gradients through the learned offsets: 5e-4)
        assert errs["out"] < 1e-4 and errs["dW"] < 1e-4 and errs["dx"] < 5e-4, errs
    else:               # tests/test_edge_cases_gpu.py
        assert errs["out"] < 1e-4 and errs["dx"] < 1e-4 and errs["dW"] < 1e-4, errs


@pytest.mark.parametrize("how", ["recycled", "in_place"])
@pytest.mark.parametrize("deformable", [False, True], ids=["rigid", "deformable"])
def test_sorted_rows_hint_does_not_outlive_its_matrix(gpu, how, deformable):
    """the sorted-rows hint of a matrix must not apply to an unsorted matrix at its recycled address, nor to the same matrix
    after an in-place change: the cut-off kernels (K3 / K6 with rows_sorted) would stop each row at its first neighbour
    beyond the kernel's reach"""
    from weasal_amd import ops
    P, U = _stale_matrix(gpu, how)
    errs = _kpconv_vs_oracle(gpu, P, U, deformable)
    _assert_bars(errs, deformable)
    assert ops.sorted_rows_radius(U) is None


def test_search_grid_does_not_outlive_an_in_place_change(gpu):
    """the table-free backward walks the search grid and never reads the index matrix: after entries of the matrix were
    overwritten in place (shadow index), dX must follow the matrix, not the grid"""
    from oracle import kpconv_ref
    from weasal_amd import config as wcfg, ops, pyramid
    from weasal_amd.kernel_points import load_kernels
    cfg = wcfg.DALESDeformF32Config()
    rng = np.random.default_rng(9)
    n = 2500
    pts = rng.uniform(-3, 3, size=(n, 3)).astype(np.float32)
    P = torch.from_numpy(pts).to(gpu)
    np.random.seed(0)
    batch = pyramid.build_batch(cfg, P, torch.ones(n, 3, device=gpu), torch.zeros(n, dtype=torch.int64, device=gpu),
                                np.array([n], np.int32), [200, 519, 472, 193, 34])
    batch.activate()
    inds = batch.neighbors[0]
    assert inds.shape == (n, 200) and ops._grid_for(inds) is not None
    with torch.no_grad():
        inds[::7, 1:6] = n                  # near neighbours of every 7th query replaced by the shadow index
    r = R_DENSE                             # kernel spanning the whole search radius: no sorted-row cut-off involved
    extent = r * cfg.KP_extent / cfg.conv_radius
    kp = torch.from_numpy(load_kernels(r, 15, dimension=3, fixed="center").astype(np.float32)).to(gpu)
    assert not ops.rows_cutoff_pays(inds, r)
    torch.manual_seed(3)
    x = torch.randn(n, CI, device=gpu, requires_grad=True)
    wf, _ = ops.kpconv_gather(x, P, P, inds, kp, extent)
    g = torch.randn_like(wf)
    dx, = torch.autograd.grad(wf, x, g)
    xc = x.detach().cpu().double().requires_grad_(True)
    Pc = P.cpu().double()
    wf_ref, _ = kpconv_ref.kpconv_gather_ref(xc, Pc, Pc, inds.cpu(), kp.cpu().double(), extent)
    dx_ref, = torch.autograd.grad(wf_ref, xc, g.cpu().double())
    assert rel(wf, wf_ref) < 1e-4
    assert rel(dx, dx_ref) < 1e-4, rel(dx, dx_ref)
    assert ops._grid_for(inds) is None


def test_col0_table_does_not_outlive_an_in_place_change(gpu):
    """closest_pool caches the transposed table of column 0; after column 0 changed in place the backward must scatter
    along the new column"""
    from weasal_amd import ops
    nc, nf, c = 3000, 20000, 64
    torch.manual_seed(7)
    x = torch.randn(nc, c, device=gpu, requires_grad=True)
    U = torch.randint(0, nc, (nf, 3), device=gpu)
    U[::11, 0] = nc                                              # shadow rows
    g = torch.randn(nf, c, device=gpu)

    def check():
        y = ops.closest_pool(x, U)
        dx, = torch.autograd.grad(y, x, g)
        real = U[:, 0] < nc
        want = torch.zeros(nc, c, dtype=torch.float64, device=gpu).index_add_(0, U[real, 0], g[real].double())
        fwd = torch.where(real[:, None], x.detach()[U[:, 0].clamp_max(nc - 1)], torch.zeros_like(y))
        assert torch.equal(y.detach(), fwd)
        assert float((dx.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())

    check()
    with torch.no_grad():
        U[:, 0] = torch.roll(U[:, 0], 1)
        U[5::13, 0] = 17
    check()


@pytest.mark.parametrize("how", ["in_place", "recycled"])
def test_demand_built_table_does_not_outlive_its_matrix(gpu, how):
    """max_pool's backward builds the full transposed table of a matrix the batch brought none for and leaves it in the
    active store; after the matrix changed in place, or was dropped and another allocated at its address, the backward must
    scatter along the new matrix.  Reference: float64 index_add_ of dy along the argmax; bar: 1e-5 of its maximum"""
    from weasal_amd import ops
    nq, h, ns, c = 2000, 8, 300, 32
    torch.manual_seed(11)
    x = torch.randn(ns, c, device=gpu, requires_grad=True)
    dy = torch.randn(nq, c, device=gpu)
    first, second = (torch.rand(nq, ns, device=gpu).argsort(dim=1)[:, :h].contiguous() for _ in range(2))      # no support twice in a row

    def check(inds):
        y = ops.max_pool(x, inds)
        dx, = torch.autograd.grad(y, x, dy)
        vals = x.detach()[inds]                                                  # [nq, h, c]
        arg = torch.gather(inds[:, :, None].expand(-1, -1, c), 1, vals.argmax(dim=1, keepdim=True))[:, 0]      # [nq, c]
        assert torch.equal(y.detach(), vals.max(dim=1).values)
        want = torch.zeros(ns * c, dtype=torch.float64, device=gpu)
        want = want.index_add_(0, (arg * c + torch.arange(c, device=gpu)).reshape(-1), dy.double().reshape(-1)).view(ns, c)
        assert float((dx.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())

    pool = torch.cuda.MemPool()             # a private pool: the next same-size request gets the freed block back
    with torch.cuda.use_mem_pool(pool):
        M = torch.empty_like(first)
    M.copy_(first)
    check(M)
    old = ops.transposed_table(M, ns)
    assert ops.transposed_table(M, ns) is old            # held for M itself
    addr, version = M.data_ptr(), M._version
    if how == "recycled":
        del M
        with torch.cuda.use_mem_pool(pool):
            U = torch.empty((nq, h), dtype=torch.int64, device=gpu)
        assert U.data_ptr() == addr          # precondition: the address of the matrix the table was built for is recycled
    else:
        U = M
    U.copy_(second)
    assert U.data_ptr() == addr and (how == "recycled" or U._version != version)
    check(U)
    assert ops.transposed_table(U, ns) is not old


# ---------------------------------------------------------------------------------------------------------------------
# ... while the fast paths still apply where they should
# ---------------------------------------------------------------------------------------------------------------------
def test_batch_hints_still_apply_to_the_batch(gpu, monkeypatch):
    """after activate() the batch's own matrices get their hints: sorted-row cut-off on every deformable level, the search
    grids (also from inside the autograd backward), the pre-built tables, the pooling orders"""
    from weasal_amd import _lib, config as wcfg, ops, pyramid
    from weasal_amd.blocks import KPConv
    cfg = wcfg.DALESDeformF32Config()
    rng = np.random.default_rng(9)
    n = 2500
    pts = rng.uniform(-3, 3, size=(n, 3)).astype(np.float32)
    P = torch.from_numpy(pts).to(gpu)
    np.random.seed(0)
    batch = pyramid.build_batch(cfg, P, torch.ones(n, 3, device=gpu), torch.zeros(n, dtype=torch.int64, device=gpu),
                                np.array([n], np.int32), [200, 519, 472, 193, 34])
    batch.activate()
    L = len(batch.points)
    for l in range(L):
        r = cfg.first_subsampling_dl * cfg.conv_radius * 2 ** l          # every level of this config is deformable
        if batch.neighbors[l].shape[0] > 0:
            assert ops.rows_cutoff_pays(batch.neighbors[l], r), l
        if l + 1 < L:
            assert ops.rows_cutoff_pays(batch.pools[l], r), l
    assert len(batch.search_grids) >= 2
    for m, grid in batch.search_grids:
        assert ops._grid_for(m) is grid
    assert batch.search_grids[0][0] is batch.neighbors[0]
    assert batch.tables and batch.col0_tables
    for inds, ns, table in batch.tables:
        assert ops.transposed_table(inds, ns) is table
    for inds, ns, table in batch.col0_tables:
        assert ops.col0_table(inds, ns) is table
    # max_pool over the batch's pooling matrix gets the cell order of its queries
    lib = _lib.lib()
    orders = []
    real_pool = lib.ws_max_pool_fwd_ordered
    monkeypatch.setattr(lib, "ws_max_pool_fwd_ordered", lambda *a: orders.append(a[8]) or real_pool(*a))
    ops.max_pool(torch.randn(n, 32, device=gpu), batch.pools[0])
    assert orders and orders[0] is not None and orders[0].value
    # the grid lookup of the backward (on the tensor autograd saved) still finds the batch's grid
    seen = []
    real_grid_for = ops._grid_for
    monkeypatch.setattr(ops, "_grid_for", lambda inds: seen.append(real_grid_for(inds)) or seen[-1])
    np.random.seed(1)
    torch.manual_seed(1)
    conv = KPConv(15, 3, CI, CO, EXT, RC).to(gpu)
    xg = torch.randn(n, CI, device=gpu, requires_grad=True)
    conv(batch.points[0], batch.points[0], batch.neighbors[0], xg).square().sum().backward()
    assert seen and seen[-1] is batch.search_grids[0][1]


def test_clear_batch_hints_drops_every_hint(gpu):
    """what KPFCNN.forward calls for a batch without activate(): nothing of the previous batch (sorted rows, grids, tables,
    pooling orders) may apply afterwards"""
    from weasal_amd import config as wcfg, ops, pyramid
    cfg = wcfg.DALESDeformF32Config()
    rng = np.random.default_rng(9)
    n = 2500
    pts = rng.uniform(-3, 3, size=(n, 3)).astype(np.float32)
    P = torch.from_numpy(pts).to(gpu)
    np.random.seed(0)
    batch = pyramid.build_batch(cfg, P, torch.ones(n, 3, device=gpu), torch.zeros(n, dtype=torch.int64, device=gpu),
                                np.array([n], np.int32), [200, 519, 472, 193, 34])
    batch.activate()
    assert ops._grid_for(batch.neighbors[0]) is not None and ops.rows_cutoff_pays(batch.neighbors[0], RC)
    ops.clear_batch_hints()
    assert ops._grid_for(batch.neighbors[0]) is None and ops.sorted_rows_radius(batch.neighbors[0]) is None
    assert ops._pool_orders_for(batch.pools[0]) == (None, None)
    assert not ops.active_hints().tables()


def test_one_route_function_serves_the_callers(gpu, monkeypatch):
    """the dX route of a KPConv backward comes from ops.dx_route: the grid walk the batch's max_count dictates on the
    self-query matrix, the transposed table on the pooling matrix (not a self-query)"""
    from weasal_amd import config as wcfg, ops, pyramid
    from weasal_amd.blocks import KPConv
    cfg = wcfg.DALESDeformF32Config()
    rng = np.random.default_rng(9)
    n = 2500
    pts = rng.uniform(-3, 3, size=(n, 3)).astype(np.float32)
    P = torch.from_numpy(pts).to(gpu)
    np.random.seed(0)
    batch = pyramid.build_batch(cfg, P, torch.ones(n, 3, device=gpu), torch.zeros(n, dtype=torch.int64, device=gpu),
                                np.array([n], np.int32), [200, 519, 472, 193, 34])
    batch.activate()
    calls = []
    real = ops.dx_route
    monkeypatch.setattr(ops, "dx_route", lambda *a, **kw: calls.append((a, real(*a, **kw))) or calls[-1][1])
    np.random.seed(1)
    torch.manual_seed(1)
    conv = KPConv(15, 3, CI, CO, EXT, RC).to(gpu)
    grid = batch.search_grids[0][1]
    assert batch.search_grids[0][0] is batch.neighbors[0] and grid.max_count > 0
    xg = torch.randn(n, CI, device=gpu, requires_grad=True)
    conv(batch.points[0], batch.points[0], batch.neighbors[0], xg).square().sum().backward()
    assert len(calls) == 1 and calls[0][0][0] is batch.neighbors[0]
    assert calls[0][1] == (ops.QUEUE_GRID if grid.max_count > ops.GRID_NARROW_MAX else ops.SLAB_GRID, grid)
    del calls[:]
    xg = torch.randn(n, CI, device=gpu, requires_grad=True)
    conv(batch.points[1], batch.points[0], batch.pools[0], xg).square().sum().backward()
    assert len(calls) == 1 and calls[0][0][0] is batch.pools[0]
    assert calls[0][1] == (ops.TABLE, None)
