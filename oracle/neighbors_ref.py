"""oracle/neighbors_ref.py -- TEST INFRASTRUCTURE ONLY.  The radius search with no search structure, in plain numpy.

oracle/geom.py (ws_oracle.cpp) is a uniform-grid search with a 3x3x3 walk like the kernels of weasal_amd/csrc/neighbors.hip
and would share a mistake in the binning, the clamping or the walk.  Here every query meets every support of its batch
element:

    diff = query - support,  d2 = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)),  hit iff d2 < fl(fl(r) * fl(r))
    key  = uint64(bits of d2) << 32 | global support index, a row is its keys in ascending order

so a row is a pure function of the input (d2 >= 0: the bit pattern is monotone; equal d2 fall back to the index).
Also here: the launcher's slab rules restated (fill_name / async_cap / fill_plan; tests hold them to the library's own
reporter, ws_radius_neighbors_fill_variant), and a parser of the exported search grid that checks it against the supports.
"""
import numpy as np

F32 = np.float32
U64 = np.uint64
ALL_ONES = U64(0xFFFFFFFFFFFFFFFF)
SLABS = (128, 576, 704, 1024, 2048)
UNSUPPORTED = "unsupported"
ENTRIES = ("search", "plan_fill", "async", "nearest")


def brute_keys(queries, supports, q_lens, s_lens, radius, chunk_pairs=1 << 22):
    """-> (keys uint64 [nq, max(count, 1)] ascending per row and padded with all ones, counts int64 [nq])"""
    q = np.ascontiguousarray(queries, dtype=F32).reshape(-1, 3)
    s = np.ascontiguousarray(supports, dtype=F32).reshape(-1, 3)
    q_lens, s_lens = np.asarray(q_lens, np.int64), np.asarray(s_lens, np.int64)
    assert q_lens.shape == s_lens.shape and q_lens.sum() == len(q) and s_lens.sum() == len(s)
    r2 = F32(radius) * F32(radius)
    counts = np.zeros(len(q), np.int64)
    rows, cols, vals = [], [], []
    q0 = s0 = 0
    for nq_b, ns_b in zip(q_lens, s_lens):
        sb = s[s0:s0 + ns_b]
        step = max(1, chunk_pairs // max(1, int(ns_b)))
        for a in range(q0, q0 + nq_b if ns_b else q0, step):
            qc = q[a:min(a + step, q0 + nq_b)]
            dx = qc[:, None, 0] - sb[None, :, 0]
            dy = qc[:, None, 1] - sb[None, :, 1]
            dz = qc[:, None, 2] - sb[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == F32
            qi, sj = np.nonzero(d2 < r2)
            k = (d2[qi, sj].view(np.uint32).astype(U64) << U64(32)) | (sj + s0).astype(U64)
            o = np.lexsort((k, qi))
            qi, k = qi[o], k[o]
            cnt = np.bincount(qi, minlength=len(qc))
            counts[a:a + len(qc)] = cnt
            rows.append(qi + a)
            cols.append(np.arange(len(qi)) - (np.cumsum(cnt) - cnt)[qi])
            vals.append(k)
        q0 += nq_b
        s0 += ns_b
    keys = np.full((len(q), max(1, int(counts.max(initial=0)))), ALL_ONES, U64)
    if rows:
        keys[np.concatenate(rows), np.concatenate(cols)] = np.concatenate(vals)
    return keys, counts


def rows(keys, counts, width, ns):
    """int64 [nq, width]: the nearest `width` supports of every query, padded with ns"""
    out = np.full((keys.shape[0], width), ns, np.int64)
    w = min(width, keys.shape[1])
    idx = (keys[:, :w] & U64(0xFFFFFFFF)).astype(np.int64)
    live = np.arange(w)[None, :] < counts[:, None]
    out[:, :w] = np.where(live, idx, ns)
    return out


def key_last(keys, counts, width):
    """uint64 [nq]: the key at sorted position width - 1 of a truncated row (count > width), all ones otherwise"""
    out = np.full(keys.shape[0], ALL_ONES, U64)
    cut = counts > width
    if cut.any():
        out[cut] = keys[cut, width - 1]
    return out


def nearest(keys, counts, ns):
    """int64 [nq]: column 0 of the row, or ns"""
    return rows(keys, counts, 1, ns)[:, 0]


# ------------------------------------------------------------------------------------------------------------------
# the launcher's rules (neighbors.hip: nb_fill_plan, ws_radius_neighbors_search, ws_radius_neighbors_async_cap)
# ------------------------------------------------------------------------------------------------------------------
def fill_slab(cap):
    for s in SLABS:
        if cap <= s:
            return s
    return 0


def fill_name(cap, out_i32=False, beside=False):
    """name of the launch that fills rows of up to `cap` neighbours (cap 0: the nearest-only kernel)"""
    t = "int32" if out_i32 else "int64"
    if cap == 0:
        return "nb_nearest_kernel<%s> grid<=4096" % t
    slab, blocks = fill_slab(cap), 1024 if beside else 4096
    if not slab:
        return UNSUPPORTED
    if slab == 128:
        return "nb_fill128_kernel<%s> grid<=%d" % (t, blocks)
    if slab == 2048:
        return "nb_fill_kernel<2048,%s> grid<=%d" % (t, blocks)
    return "nb_fill_wide_kernel<%s,%d> grid<=%d" % (t, slab, blocks)


def async_cap(width, wide_caps=1):
    """slab of the asynchronous search for rows of `width` entries: 5/4 of the width, rounded up to a kernel variant"""
    if width <= 128:
        return 128
    if not wide_caps:
        return 1024
    need = width + width // 4
    return 576 if need <= 576 else 704 if need <= 704 else 1024


def fill_caps(entry, width, max_count, wide_caps=1):
    """caps of the fill launches an entry makes, in order; None stands for the refused launch above 2048"""
    if entry == "nearest":
        return [0]
    if entry == "plan_fill":            # the plan counts, the fill is sized to the count
        return [] if max_count == 0 else [max_count if max_count <= 2048 else None]
    if entry == "search":               # first pass by the width asked for, one more pass when a row overflowed it
        caps = [1024 if width > 128 else 128]
        if max_count > caps[0]:
            caps.append(max_count if max_count <= 2048 else None)
        return caps
    if entry == "async":                # one pass; an overflow is reported and DeferredSearches.finish repeats through "search"
        caps = [async_cap(width, wide_caps)]
        return caps + (fill_caps("search", width, max_count) if max_count > caps[0] else [])
    raise ValueError(entry)


def fill_plan(entry, width, max_count, wide_caps=1, out_i32=False):
    """the launches `entry` makes for rows of `width` entries when the longest row holds max_count, as fill_name strings"""
    caps = fill_caps(entry, width, max_count, wide_caps)
    return [UNSUPPORTED if c is None else fill_name(c, out_i32, beside=(entry == "async" and i == 0))
            for i, c in enumerate(caps)]


# ------------------------------------------------------------------------------------------------------------------
# the exported grid (ws_grid.h: [CloudGrid nb | cell_start cells + 2 | float4 sorted ns], sections 256-byte aligned)
# ------------------------------------------------------------------------------------------------------------------
CLOUD_GRID = np.dtype([("lo", "<f4", 3), ("inv_cell", "<f4"), ("nx", "<i4"), ("ny", "<i4"), ("nz", "<i4"), ("cell_base", "<i4"),
                       ("cell_cap", "<i4"), ("s_base", "<i4"), ("s_len", "<i4"), ("q_base", "<i4"), ("q_len", "<i4")])
MAX_DIM = 512


def _align(b):
    return (b + 255) // 256 * 256


def parse_grid(blob, nb, cells, ns):
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    c_off = _align(nb * CLOUD_GRID.itemsize)
    s_off = c_off + _align((cells + 2) * 4)
    assert blob.size == s_off + 16 * ns, (blob.size, s_off + 16 * ns)
    grids = blob[:nb * CLOUD_GRID.itemsize].view(CLOUD_GRID)
    cell_start = blob[c_off:c_off + 4 * (cells + 1)].view("<i4")
    entries = blob[s_off:s_off + 16 * ns].view("<f4").reshape(ns, 4)
    return grids, cell_start, entries


def cell_coord(v, lo, inv):
    """the float32 recipe of ws_grid.h: floor((v - lo) * inv), kept inside [-2, 1e6] before the conversion"""
    t = np.floor((v.astype(F32) - F32(lo)) * F32(inv))
    return np.minimum(np.maximum(t, F32(-2.0)), F32(1.0e6)).astype(np.int64)


def cell_cap(s_len):
    return 4 * int(s_len) + 64


def grid_dims(lo, hi, radius, s_len):
    """nb_grid_setup_kernel restated: -> (number of growth steps, (nx, ny, nz)); the cell starts at 1.001 r and grows by
    1.26 until every dimension is <= 512 and the element fits its 4 s_len + 64 cells"""
    cell = (F32(radius) if radius > 0 else F32(1)) * F32(1.001)
    steps = 0
    while True:
        inv = F32(1) / cell
        dims = tuple(int(np.floor((F32(h) - F32(l)) * inv)) + 1 for l, h in zip(lo, hi))
        if max(dims) <= MAX_DIM and dims[0] * dims[1] * dims[2] <= cell_cap(s_len):
            return steps, dims
        cell = cell * F32(1.26)
        steps += 1


def check_grid(blob, nb, cells, ns, order, supports, s_lens, radius):
    """asserts that an exported grid files every support of every element under the cell its coordinates name; returns the
    per-element records"""
    s = np.ascontiguousarray(supports, dtype=F32).reshape(-1, 3)
    s_lens = np.asarray(s_lens, np.int64)
    assert nb == len(s_lens) and ns == len(s) == s_lens.sum()
    assert cells == sum(cell_cap(n) for n in s_lens)
    grids, cell_start, entries = parse_grid(blob, nb, cells, ns)
    assert cell_start[0] == 0 and cell_start[cells] == ns and np.all(np.diff(cell_start) >= 0)
    index = entries[:, 3].copy().view("<i4").astype(np.int64)
    assert np.array_equal(np.sort(index), np.arange(ns))
    assert np.array_equal(entries[:, :3].view("<u4"), s[index].view("<u4"))
    if order is not None:
        assert np.array_equal(np.asarray(order, np.int64), index)
    filed = np.searchsorted(cell_start[:cells + 1], np.arange(ns), side="right") - 1
    s_base = cell_base = 0
    for b, g in enumerate(grids):
        n = int(s_lens[b])
        assert (g["s_base"], g["s_len"], g["cell_base"], g["cell_cap"]) == (s_base, n, cell_base, cell_cap(n)), (b, g)
        assert cell_start[cell_base] == s_base and cell_start[cell_base + cell_cap(n)] - cell_start[cell_base] == n, b
        nx, ny, nz = int(g["nx"]), int(g["ny"]), int(g["nz"])
        if n == 0:
            assert (nx, ny, nz) == (1, 1, 1) and g["inv_cell"] == F32(1) and not g["lo"].any(), (b, g)
        else:
            assert F32(g["inv_cell"]) * F32(radius) < F32(1), (b, g)
            assert 1 <= min(nx, ny, nz) and max(nx, ny, nz) <= MAX_DIM and nx * ny * nz <= cell_cap(n), (b, g)
            e = entries[s_base:s_base + n]
            assert np.all((index[s_base:s_base + n] >= s_base) & (index[s_base:s_base + n] < s_base + n)), b
            assert np.array_equal(g["lo"], s[s_base:s_base + n].min(0)), (b, g)
            cx = np.clip(cell_coord(e[:, 0], g["lo"][0], g["inv_cell"]), 0, nx - 1)
            cy = np.clip(cell_coord(e[:, 1], g["lo"][1], g["inv_cell"]), 0, ny - 1)
            cz = np.clip(cell_coord(e[:, 2], g["lo"][2], g["inv_cell"]), 0, nz - 1)
            assert np.array_equal(filed[s_base:s_base + n], cell_base + (cz * ny + cy) * nx + cx), b
        s_base += n
        cell_base += cell_cap(n)
    same_cell = filed[1:] == filed[:-1]
    assert np.all(index[1:][same_cell] > index[:-1][same_cell])        # indices ascend inside every cell
    return grids
