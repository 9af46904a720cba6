"""CPU: the one store of index hints (weasal_amd/hints.py), its thin reads in ops, and ops.dx_route.

The store's rule needs no device: a hint answers only for the tensor object it was registered with, at the version it had.
Index matrices are CPU tensors of 4 x 3, payloads are plain objects.
"""
import gc
import itertools
import types

import pytest
import torch

from weasal_amd import ops
from weasal_amd.hints import BatchHints

NS = 7
# kind -> (keywords of BatchHints.add, arguments of BatchHints.get after the matrix)
KINDS = {
    "radius": (dict(radius=2.5), ("radius",)),
    "grid": (dict(grid=object()), ("grid",)),
    "pool_orders": (dict(pool_orders=(object(), object())), ("pool_orders",)),
    "table": (dict(ns=NS, table=object()), ("table", NS)),
    "col0_table": (dict(ns=NS, col0_table=object()), ("col0_table", NS)),
}


def _matrix():
    return torch.arange(12, dtype=torch.int64).reshape(4, 3).clone()


def _payload(kind):
    kw = KINDS[kind][0]
    return kw[kind]


@pytest.fixture(autouse=True)
def _fresh_store():
    ops.clear_batch_hints()
    yield
    ops.clear_batch_hints()


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_hint_answers_only_for_its_own_tensor(kind):
    store = BatchHints()
    kw, key = KINDS[kind]
    M = _matrix()
    store.add(M, **kw)
    assert store.get(M, *key) is _payload(kind)
    alias = M.view_as(M)                        # another object: same address, shape and version
    assert alias is not M and alias.data_ptr() == M.data_ptr() and alias._version == M._version
    assert store.get(alias, *key) is None
    M.add_(0)                                   # same object, bumped version
    assert store.get(M, *key) is None
    store.add(M, **kw)
    assert store.get(M, *key) is _payload(kind) and store.n_matrices() == 1
    del M, alias
    gc.collect()
    N = _matrix()                               # registered under nothing (wherever the allocator put it)
    assert store.get(N, *key) is None
    other = _matrix()
    store.add(other, radius=1.0)                # the next insert drops the dead tensor's entry
    assert store.n_matrices() == 1 and store.get(other, "radius") == 1.0
    assert store.get(N, *key) is None


@pytest.mark.parametrize("first", list(KINDS))
def test_kinds_are_independent(first):
    store = BatchHints()
    M = _matrix()
    store.add(M, **KINDS[first][0])
    for kind, (_, key) in KINDS.items():
        assert (store.get(M, *key) is not None) == (kind == first), kind
    assert store.get(M, "table", NS + 1) is None and store.get(M, "col0_table", NS + 1) is None      # tables are per ns
    for second in KINDS:
        store.add(M, **KINDS[second][0])        # a second kind keeps the first
        assert store.get(M, *KINDS[first][1]) is _payload(first)
        assert store.get(M, *KINDS[second][1]) is _payload(second)


def _full_store():
    store = BatchHints()
    M, P = _matrix(), torch.zeros(5, 3)
    for kw, _ in KINDS.values():
        store.add(M, **kw)
    store.add_point_order(P, torch.arange(5, dtype=torch.int32))
    return store, M, P


def _reads(M, P):
    """what the operators see of (M, P) through the active store; tables through the store itself (building one needs a GPU)"""
    active = ops.active_hints()
    return [ops.sorted_rows_radius(M), ops._grid_for(M), active.get(M, "pool_orders"), active.get(M, "table", NS),
            active.get(M, "col0_table", NS), ops._order_for(P)]


def test_install_and_clear_replace_everything():
    first, M1, P1 = _full_store()
    second, M2, P2 = _full_store()
    ops.install_hints(first)
    assert all(v is not None for v in _reads(M1, P1))
    assert ops.rows_cutoff_pays(M1, 2.0) and not ops.rows_cutoff_pays(M1, 2.2)      # 2.5 > 1.2 r
    ops.install_hints(second)
    assert all(v is None for v in _reads(M1, P1))
    assert all(v is not None for v in _reads(M2, P2))
    ops.clear_batch_hints()
    assert all(v is None for v in _reads(M2, P2))
    assert ops._pool_orders_for(M2) == (None, None)
    assert not ops.active_hints().tables() and ops.active_hints().n_matrices() == 0
    assert all(v is not None for v in [first.get(M1, "grid"), second.get(M2, "grid")])      # the batches keep their own


def test_switches_hide_grids_and_radii(monkeypatch):
    store, M, _ = _full_store()
    ops.install_hints(store)
    assert ops._grid_for(M) is not None and ops.sorted_rows_radius(M) == 2.5
    monkeypatch.setattr(ops, "GRID_BACKWARD", False)
    assert ops._grid_for(M) is None and ops.sorted_rows_radius(M) == 2.5
    monkeypatch.setattr(ops, "GRID_BACKWARD", True)
    monkeypatch.setattr(ops, "SORTED_ROW_CUTOFF", False)
    assert ops._grid_for(M) is not None and ops.sorted_rows_radius(M) is None and not ops.rows_cutoff_pays(M, 1.0)


def test_orders_that_do_not_fit_are_not_returned():
    P = torch.zeros(5, 3)
    order = torch.arange(5, dtype=torch.int32)
    ops.register_point_order(P, order)
    assert ops._order_for(P) is order
    assert ops._order_for(P.detach()) is order           # by address: the operators pass a detached alias of the batch's points
    ops.register_point_order(P, torch.arange(4, dtype=torch.int32))
    assert ops._order_for(P) is None                     # wrong length
    ops.register_point_order(P, order.to("meta"))
    assert ops._order_for(P) is None                     # wrong device
    M = _matrix()
    oq, osup = torch.arange(4, dtype=torch.int32), torch.arange(NS, dtype=torch.int32)
    ops.active_hints().add(M, pool_orders=(oq, osup))
    got = ops._pool_orders_for(M, NS)
    assert got[0] is oq and got[1] is osup
    got = ops._pool_orders_for(M, NS + 1)
    assert got[0] is oq and got[1] is None
    ops.active_hints().add(M, pool_orders=(osup, oq))
    assert ops._pool_orders_for(M, NS) == (None, None)


@pytest.mark.parametrize("what", ["empty", "one_dim", "no_tensor"])
def test_only_a_matrix_with_rows_is_registered(what):
    store = BatchHints()
    m = {"empty": torch.zeros((0, 1), dtype=torch.int64), "one_dim": torch.zeros(4, dtype=torch.int64), "no_tensor": None}[what]
    for kw, _ in KINDS.values():
        store.add(m, **kw)
    assert store.n_matrices() == 0 and not store.tables()


def test_bound_on_demand_built_tables(monkeypatch):
    built = []

    class Stub:
        def __init__(self, inds, ns):
            built.append((inds.data_ptr(), ns))

    monkeypatch.setattr(ops, "TransposedTable", Stub)
    brought = _matrix()
    ops.active_hints().add(brought, NS, table="brought")      # a table the batch brought does not count against the bound
    bound = BatchHints.TABLES_MAX
    mats = [_matrix() for _ in range(bound + 3)]
    tables = [ops.transposed_table(m, NS) if i % 2 else ops.col0_table(m, NS) for i, m in enumerate(mats)]
    assert len(built) == len(mats)
    assert len(ops.active_hints().tables()) == bound + 1
    for i, m in enumerate(mats):
        held = ops.active_hints().get(m, "table" if i % 2 else "col0_table", NS)
        assert held is (tables[i] if i >= 3 else None), i      # the oldest three are gone
    assert ops.transposed_table(mats[-2], NS) is tables[-2] and len(built) == len(mats)      # a hit builds nothing
    assert ops.transposed_table(brought, NS) == "brought"
    assert ops.transposed_table(mats[1], NS) is not tables[1] and len(built) == len(mats) + 1      # an evicted one is rebuilt
    # a dead matrix's table leaves with it, at the next insert
    n, entries = len(ops.active_hints().tables()), ops.active_hints().n_matrices()
    del mats[-1], m
    gc.collect()
    ops.col0_table(brought, NS)
    assert ops.active_hints().n_matrices() == entries - 1
    assert len(ops.active_hints().tables()) == n           # one dead, one new, and the dead one made room under the bound
    ops.clear_table_cache()
    assert not ops.active_hints().tables()


# ---------------------------------------------------------------------------------------------------------------------
# ops.dx_route against the three sites it replaced, written out from them case by case:
#   _KPConvGather.backward     grid only for a self-query; rows > 128 and not rigid linear / sum -> no grid; with a grid of the
#                              right ns: rows > 128 -> queue form, else slab form; otherwise the table
#   _KPConvGatherDef.backward  grid only for a self-query; with a grid of the right ns the queue form, otherwise the table
#   fused._geometry            grid only for a self-query, of the right ns and with rows <= 128: slab form; otherwise the table
# ---------------------------------------------------------------------------------------------------------------------
S, Q, T = "slab grid walk", "queue grid walk", "transposed table"
# (caller, max_count of the grid, rigid linear / sum) -> route, for a self-query whose grid is visible and has the right ns
WITH_GRID = {
    ("generic", 128, True): S, ("generic", 128, False): S, ("generic", 129, True): Q, ("generic", 129, False): T,
    ("packed", 128, True): Q, ("packed", 128, False): Q, ("packed", 129, True): Q, ("packed", 129, False): Q,
    ("block", 128, True): S, ("block", 128, False): S, ("block", 129, True): T, ("block", 129, False): T,
}
GRIDS = ["absent", 128, 129, "ns_mismatch_128", "ns_mismatch_129"]
NOT_RIGID_LINEAR_SUM = ["deformed", "modulated", "constant", "gaussian", "closest"]


@pytest.mark.parametrize("caller", ["generic", "packed", "block"])
def test_dx_route_matches_the_three_sites(caller, monkeypatch):
    assert (ops.SLAB_GRID, ops.QUEUE_GRID, ops.TABLE) == (S, Q, T) and ops.GRID_NARROW_MAX == 128
    n = 4
    P = torch.zeros(n, 3)
    other = torch.zeros(n, 3)              # as many queries as supports, another tensor: not a self-query
    cases = 0
    for self_query, grid_case, variant, grid_backward in itertools.product(
            [True, False], GRIDS, ["rigid_linear_sum"] + NOT_RIGID_LINEAR_SUM, [True, False]):
        monkeypatch.setattr(ops, "GRID_BACKWARD", grid_backward)
        ops.clear_batch_hints()
        M = _matrix()
        grid = None
        if grid_case != "absent":
            mismatch = isinstance(grid_case, str)
            grid = types.SimpleNamespace(ns=n + 1 if mismatch else n, max_count=int(str(grid_case)[-3:]))
            ops.active_hints().add(M, grid=grid)
        # what the generic operator derives its flag from (ops._KPConvGather.backward): dkp, mod, influence, aggregation
        dkp = object() if variant == "deformed" else None
        mod = object() if variant == "modulated" else None
        influence = ops.INFLUENCE.get(variant, 0)
        aggregation = ops.AGGREGATION.get(variant, 0)
        plain = dkp is None and mod is None and influence == 0 and aggregation == 0
        assert plain == (variant == "rigid_linear_sum")
        live = self_query and grid_backward and grid_case in (128, 129)
        want = WITH_GRID[(caller, grid_case, plain)] if live else T
        route, got_grid = ops.dx_route(M, P, P if self_query else other, caller, plain)
        assert route == want, (caller, self_query, grid_case, variant, grid_backward, route)
        assert got_grid is (grid if want != T else None)
        cases += 1
    assert cases == 2 * 5 * 6 * 2


def test_dx_route_needs_as_many_queries_as_supports():
    M = _matrix()
    ops.active_hints().add(M, grid=types.SimpleNamespace(ns=4, max_count=10))
    P = torch.zeros(4, 3)
    assert ops.dx_route(M, P, P, "generic") == (S, ops._grid_for(M))
    assert ops.dx_route(M, P[:3], P, "generic") == (T, None)      # same address, fewer queries
