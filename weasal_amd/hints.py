"""What one batch knows about its index matrices and point sets beyond their values: the state that chooses a kernel path
without being an argument of any call.

A hint about an index matrix answers only for the tensor object it was registered with, at the `_version` it had then.  A
matrix built later at a recycled address, or the same matrix changed in place, gets nothing: a stale hint makes the kernels
walk the wrong rows without any error (tests/test_stale_state_gpu.py).  The rule is `BatchHints.get`; every kind of index hint
goes through it.  The reference to the tensor is weak, so the store neither keeps a matrix alive nor its address from being
recycled.
"""
import weakref

KINDS = ("radius", "grid", "pool_orders", "table", "col0_table")


class BatchHints:
    """Per index matrix [Nq, H]:
      radius       the search radius its rows were sorted for (rows sorted by distance from the query);
      grid         the ops.SearchGrid of the self-query search that wrote it (table-free KPConv backward);
      pool_orders  (cell order of its queries or None, cell order of its supports or None): scheduling of ops.max_pool;
      table        its transposed table over `ns` supports, one per ns;
      col0_table   the transposed table of its first column over `ns` supports, one per ns.
    Per point set: its scheduling order (a spatially coherent permutation, the cell order of the neighbour search)."""

    TABLES_MAX = 32      # tables built on demand (transposed_table / col0_table on a matrix the batch brought no table for)

    def __init__(self):
        self._index = {}        # (data_ptr, shape) -> (weakref of the matrix, its _version, {kind or (kind, ns): payload})
        self._orders = {}       # points.data_ptr() -> order
        self._on_demand = []    # (fields of an entry, key in them) of the tables built on demand, oldest first

    def _fields(self, inds):
        hit = self._index.get((inds.data_ptr(), tuple(inds.shape)))
        if hit is None or hit[0]() is not inds or hit[1] != inds._version:
            return None
        return hit[2]

    def get(self, inds, kind, ns=None):
        """the `kind` hint registered for `inds` itself at its current version, else None"""
        fields = self._fields(inds)
        return None if fields is None else fields.get(kind if ns is None else (kind, ns))

    def add(self, inds, ns=None, on_demand=False, **hints):
        """register hints (keywords: KINDS; the two tables need `ns`) for one index matrix, next to what is already known about
        that same tensor.  Anything but a 2-D tensor with rows is not registrable.  on_demand: the table was built because
        somebody asked, not brought by the batch; at most TABLES_MAX of those are held, the oldest go first."""
        if not (hasattr(inds, "data_ptr") and inds.dim() == 2 and inds.shape[0] > 0):
            return
        # entries of dead tensors go at the next insert, not at the next batch (a weak entry pins no index matrix in device
        # memory: all there is to drop is its tables)
        self._index = {k: e for k, e in self._index.items() if e[0]() is not None}
        fields = self._fields(inds)
        if fields is None:
            fields = {}
            self._index[(inds.data_ptr(), tuple(inds.shape))] = (weakref.ref(inds), inds._version, fields)
        for kind, payload in hints.items():
            assert kind in KINDS, kind
            key = (kind, ns) if kind in ("table", "col0_table") else kind
            fields[key] = payload
            if on_demand:
                self._on_demand.append((fields, key))
        if on_demand:
            live = {id(e[2]) for e in self._index.values()}
            self._on_demand = [d for d in self._on_demand if id(d[0]) in live]
            while len(self._on_demand) > self.TABLES_MAX:
                old, key = self._on_demand.pop(0)
                old.pop(key, None)

    def n_matrices(self):
        """index matrices the store holds an entry for"""
        return len(self._index)

    def drop_tables(self):
        for _, _, fields in self._index.values():
            for key in [k for k in fields if isinstance(k, tuple)]:
                del fields[key]
        self._on_demand = []

    def tables(self):
        """every table held, of either kind (tests)"""
        return [p for _, _, fields in self._index.values() for k, p in fields.items() if isinstance(k, tuple)]

    # Point orders are keyed by address on purpose: the operators hand the kernels a detached float32 alias of the batch's
    # point tensor (ops._f32c), so object identity cannot match.  That is sound here and only here: the order is a valid
    # permutation that the store keeps alive, and the result of every kernel is independent of it.
    def add_point_order(self, points, order):
        self._orders[points.data_ptr()] = order

    def order_for(self, points):
        o = self._orders.get(points.data_ptr())
        if o is not None and o.numel() == points.shape[0] and o.device == points.device:
            return o
        return None
