"""oracle/subsample_ref.py -- TEST INFRASTRUCTURE ONLY (numpy).

Independent description of grid subsampling (weasal_amd/csrc/subsample.hip) for tests/test_subsample_branches_*.py, plus the
named data sets and case tables both files share.

What is restated here, in float32 numpy, from grid_subsampling.cpp:25-31, :53-68, :87-94:
  origin  inv = f32(1) / dl; org = floor(min * inv) * dl; nX = (size_t)floor((max.x - org.x) / dl) + 1, nY alike
  key     iX + nX * iY + nX * nY * iZ mod 2^64, i = (size_t)floor((p - org) / dl) (x86-64: through int64, negatives wrap)
  cell    members in input order; running f32 sums; barycentre sum * f32(1.0 / count); feature mean sum / f32(count);
          one label histogram per label column

This says WHICH rows exist and what they hold.  Row ORDER (the iteration order of an std::unordered_map<size_t, .>) and the
label of a cell whose histogram has several maxima (the iteration order of an std::unordered_map<int, int>) are not restated:
they come from the port oracle alone (oracle/ws_oracle.cpp through oracle/geom.py).

Data sets (at most 8193 points each):
  lattice<m>       exactly m occupied cells, 3 points per cell on average, shuffled; dl = 0.25 and offsets that are multiples
                   of it, so the count is exact
  rounding<dl>     four elements: points on and one ulp either side of k dl (both f32(k) * dl and f32(k * dl)); all floats
                   of a stretch near 4e5, where the f32 spacing (1/32) is a sizeable fraction of dl; negative coordinates;
                   an element whose minimum is an edge value above which the origin rounds (where dl has one)
  wrapped_key      dl = 0.1f with min.x = f32(0.9): the origin 0.90000004 lies ABOVE the minimum, iX = (size_t)-1, and the
                   point in y-cell 0, z-cell 0 has the key 2^64 - 1 (the GPU hash table's reserved value); 61 cells
  crowded          4096 points in one cell and a few single-point cells, three feature columns
  labels_many      cells with exactly 13, 14, 29, 30 and 48 distinct labels (either side of the histogram map's rehashes and
                   at the size of the kernel's per-thread histogram), three labels tied for the maximum, negative labels
  labels_overflow  cells with 49, 60 and 130 distinct labels: unique maxima first seen after the 48th label, and ties
  emit             two elements of 30 and 14 cells with five feature and three label columns (few classes: ties abound)
  scan<n>          n points in one element; scan_small: elements of 32, 33 and 1 points
"""
import zlib

import numpy as np

ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
MAXL = 48                                    # per-thread label histogram of sub_emit_labels_kernel

# cell counts either side of every rehash of the cell map (13|14 ... 2357|2358) and of the 1024-item chunk of the block scan
ROW_COUNTS = (1, 2, 13, 14, 29, 30, 59, 60, 127, 128, 257, 258, 541, 542, 1024, 1025, 1109, 1110, 2357, 2358)
# one batch: empty elements first, twice in a row in the middle, and last
MIXED_COUNTS = (0, 14, 13, 0, 0, 60, 258, 1, 1025, 0)
ROUNDING_DLS = (0.1, 0.3, 0.06, 0.48)
SCAN_N = (1, 4095, 4096, 4097, 8193)
LABEL_CELL_SIZES = (13, 14, 29, 30, 48)
OVERFLOW_CELL_SIZES = (49, 60, 130)
EMIT_M = (30, 14)
EMIT_FD = (1, 3, 5)
EMIT_LD = ("1d", 1, 2, 3)                    # "1d": a one-dimensional label tensor
EMIT_MAX_P = (0, 7, EMIT_M[0], EMIT_M[0] + 1)
LATTICE_DL = 0.25


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------------------------------
# cell keys and cell contents
# ------------------------------------------------------------------------------------------------------------------
def _cell_index(x, org, dl):
    """(size_t)floor((x - org) / dl) of x86-64: float -> int64 -> uint64"""
    return np.floor((x - org) / dl).astype(np.int64).astype(np.uint64)


def cell_keys(points, dl):
    """uint64 [n] cell key of every point of ONE element"""
    p = np.ascontiguousarray(points, dtype=np.float32)
    dl = np.float32(dl)
    if len(p) == 0:
        return np.zeros(0, np.uint64)
    inv = np.float32(1) / dl
    mn, mx = p.min(0), p.max(0)
    org = np.floor(mn * inv) * dl
    assert org.dtype == np.float32
    with np.errstate(over="ignore"):
        nx = _cell_index(mx[0:1], org[0], dl) + np.uint64(1)
        ny = _cell_index(mx[1:2], org[1], dl) + np.uint64(1)
        ix, iy, iz = (_cell_index(p[:, d], org[d], dl) for d in range(3))
        return ix + nx * iy + nx * ny * iz


def _running_sum(x):
    """sequential float32 sum down the rows, like `sum += x` in input order"""
    return np.add.accumulate(np.ascontiguousarray(x, dtype=np.float32), axis=0, dtype=np.float32)[-1]


def cells(points, lens, dl, features=None, labels=None):
    """per element: dict(keys, first, members, counts, bary[, fmean][, hist]); cells in first-occurrence order.
    hist[cell][column] = {label: count}, labels in first-seen order."""
    p = np.ascontiguousarray(points, dtype=np.float32)
    f = None if features is None else np.ascontiguousarray(features, dtype=np.float32)
    c = None if labels is None else np.ascontiguousarray(labels, dtype=np.int32).reshape(len(p), -1)
    out, i0 = [], 0
    for n in np.asarray(lens):
        n = int(n)
        pe = p[i0:i0 + n]
        k = cell_keys(pe, dl)
        uniq, first, inv = np.unique(k, return_index=True, return_inverse=True)
        by_first = np.argsort(first, kind="stable")
        rank = np.empty(len(uniq), np.int64)
        rank[by_first] = np.arange(len(uniq))
        cell_of = rank[inv.reshape(-1)] if n else np.zeros(0, np.int64)
        order = np.argsort(cell_of, kind="stable")                    # members of a cell stay in input order
        counts = np.bincount(cell_of, minlength=len(uniq)).astype(np.int32)
        ends = np.cumsum(counts)
        members = [order[e - m:e] for e, m in zip(ends, counts)]
        e = dict(keys=uniq[by_first], first=first[by_first], members=members, counts=counts)
        e["bary"] = np.array([_running_sum(pe[m]) * np.float32(1.0 / len(m)) for m in members], np.float32).reshape(-1, 3)
        if f is not None:
            fe = f[i0:i0 + n]
            e["fmean"] = np.array([_running_sum(fe[m]) / np.float32(len(m)) for m in members], np.float32).reshape(-1, f.shape[1])
        if c is not None:
            ce = c[i0:i0 + n]
            e["hist"] = [[_histogram(ce[m, col]) for col in range(c.shape[1])] for m in members]
        out.append(e)
        i0 += n
    assert i0 == len(p)
    return out


def _histogram(values):
    h = {}
    for v in values.tolist():
        h[v] = h.get(v, 0) + 1
    return h


def first_seen_rows(ref_cells, port_keys, port_lens):
    """index of the port's rows (no max_p) that puts every element into first-seen order: row i of element b becomes the
    cell whose earliest point comes i-th.  The key sets of both sides must agree."""
    idx, r0 = [], 0
    for e, m in zip(ref_cells, port_lens):
        m = int(m)
        pk = np.asarray(port_keys[r0:r0 + m])
        assert len(e["keys"]) == m and len(set(pk.tolist())) == m
        where = {int(k): r0 + i for i, k in enumerate(pk.tolist())}
        idx += [where[int(k)] for k in e["keys"].tolist()]
        r0 += m
    return np.asarray(idx, np.int64)


# ------------------------------------------------------------------------------------------------------------------
# data sets
# ------------------------------------------------------------------------------------------------------------------
def _data(p, lens, dl, f=None, c=None, **extra):
    p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 3)
    d = dict(p=p, lens=np.asarray(lens, np.int32), dl=float(np.float32(dl)), f=None, c=None, **extra)
    if f is not None:
        d["f"] = np.ascontiguousarray(f, dtype=np.float32)
    if c is not None:
        d["c"] = np.ascontiguousarray(c, dtype=np.int32)
    assert int(d["lens"].sum()) == len(p)
    for a in (d["p"], d["lens"], d["f"], d["c"]):
        if a is not None:
            a.setflags(write=False)
    return d


def lattice_points(rng, m, per, dl=LATTICE_DL, offset=(0.0, 0.0, 0.0)):
    """points of exactly m occupied cells (per points per cell on average, every cell at least one), shuffled.  dl is exact
    in binary and offset a multiple of it; the points keep a tenth of a cell from every face."""
    if m == 0:
        return np.zeros((0, 3), np.float32)
    assert (np.asarray(offset) / dl == np.round(np.asarray(offset) / dl)).all()
    side = int(np.ceil(m ** (1.0 / 3.0))) + 1
    chosen = rng.choice(side ** 3, size=m, replace=False)
    cell = np.stack(np.unravel_index(chosen, (side, side, side)), 1)
    owner = np.concatenate([np.arange(m), rng.integers(0, m, size=m * (per - 1))])
    pts = (cell[owner] + rng.uniform(0.1, 0.9, size=(len(owner), 3))) * dl + np.asarray(offset)
    return pts[rng.permutation(len(pts))].astype(np.float32)


def lattice(m, per=3, dl=LATTICE_DL, offset=(0.0, 0.0, 0.0)):
    return _data(lattice_points(_rng("lattice", m, per, offset), m, per, dl, offset), [m * per], dl, m=[m])


def mixed(counts=MIXED_COUNTS, per=3):
    """one batch of lattices, each at an offset of its own; zero = an empty element"""
    rng = _rng("mixed", counts)
    parts = [lattice_points(rng, m, per, LATTICE_DL, (LATTICE_DL * 4 * b, -LATTICE_DL * 8 * b, LATTICE_DL * b))
             for b, m in enumerate(counts)]
    return _data(np.concatenate(parts), [len(a) for a in parts], LATTICE_DL, m=list(counts))


def _neighbours(v):
    v = np.asarray(v, np.float32)
    return np.concatenate([np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))])


def rounding(dl):
    rng = _rng("rounding", dl)
    d32 = np.float32(dl)
    k = np.arange(0, 48)
    edges = np.unique(np.concatenate([_neighbours(k.astype(np.float32) * d32), _neighbours((k * float(dl)).astype(np.float32))]))

    def cloud(values_x, values_yz, n):
        x = values_x[rng.integers(0, len(values_x), size=n)]
        yz = values_yz[rng.integers(0, len(values_yz), size=(n, 2))]
        pts = np.concatenate([x[:, None], yz], 1)
        pts[:len(values_x), 0] = values_x                              # every edge value occurs
        return pts[rng.permutation(n)].astype(np.float32)

    near = cloud(edges, edges[:18], 700)
    # around 4e5 every float32 is a multiple of 1/32: all of them over a stretch of a few cells
    span = np.float32(4e5) + np.arange(0, 160, dtype=np.float32) / np.float32(32)
    far = cloud(span, span[:48], 700) + np.asarray([0, 1000, -8e5], np.float32)
    neg = -cloud(edges, edges[:18], 700)
    # an element whose minimum is itself an edge value v with floor(v * (1 / dl)) * dl > v, where there is one: the origin
    # then lies above the minimum and cell indices of -1 occur on every axis
    inv = np.float32(1) / d32
    above = edges[(np.floor(edges * inv) * d32 > edges) & (edges > 0)]
    v0 = above[0] if len(above) else edges[4]
    tail = edges[edges >= v0]
    up = cloud(tail, tail[:18], 700)
    return _data(np.concatenate([near, far, neg, up]), [700, 700, 700, 700], dl, origin_above=len(above) > 0)


WRAPPED_X0 = np.float32(0.9)                 # 0.8999999761581421: floor(x0 * (1 / 0.1f)) * 0.1f = 0.90000004 > x0
WRAPPED_SEED = 0


def wrapped_key(seed=WRAPPED_SEED, drop_wrapped=False, move_wrapped=False):
    """61 cells of dl = 0.1f; the first point has the key 2^64 - 1.  drop_wrapped leaves that point out: a second point with
    x = x0 keeps the origin where it was, and 60 cells stay (still past the 59|60 rehash).  move_wrapped lifts it one cell in
    z instead: the same 61 cells in the same order of first occurrence, only that one key differs."""
    rng = _rng("wrapped_key", seed)
    dl = np.float32(0.1)
    # cells: the wrapped one, one more with iX = -1 (j == 0 below), 58 of the 8 x 8 block, and (0, 0) with the pinning point.
    # The key of (iX = -1, iY) is that of (nX - 1, iY - 1): the second such cell sits in row 9, above an empty row 8.
    cellsxy = rng.choice(np.arange(1, 64), size=59, replace=False)
    pts = [(WRAPPED_X0, 0.05, 0.05)]                                   # iX = -1, iY = iZ = 0
    for j, cxy in enumerate(cellsxy):
        ix, iy = int(cxy) % 8, int(cxy) // 8
        for _ in range(1 + int(rng.integers(0, 3))):
            x = WRAPPED_X0 if j == 0 else 0.9 + (ix + rng.uniform(0.3, 0.7)) * 0.1
            pts.append((x, ((9 if j == 0 else iy) + rng.uniform(0.3, 0.7)) * 0.1,
                        rng.uniform(0.03, 0.07)))
    pts = np.asarray(pts, np.float32)
    pts[1:] = pts[1:][rng.permutation(len(pts) - 1)]
    pts = np.concatenate([pts, np.asarray([(0.95, 0.0, 0.0)], np.float32)])       # pins min.y = min.z = 0 inside a cell above
    if move_wrapped:
        pts[0, 2] += np.float32(0.1)
    if drop_wrapped:
        pts = pts[1:]
    return _data(pts, [len(pts)], dl)


def crowded():
    rng = _rng("crowded")
    big = rng.uniform(0.01, 0.49, size=(4096, 3)) + (1.0, 0.5, 0.0)
    singles = np.asarray([(0.2, 0.2, 0.2), (2.3, 0.1, 0.4), (1.2, 1.7, 0.3), (0.1, 2.2, 1.8), (2.7, 2.7, 2.7)])
    pts = np.concatenate([big, singles])
    perm = rng.permutation(len(pts))
    f = rng.normal(size=(len(pts), 3)) * (1.0, 100.0, 1e-3) + (0.0, 50.0, 0.0)
    return _data(pts[perm], [len(pts)], 0.5, f=f)


def _label_cell(rng, distinct, pattern):
    """label sequence of one cell with `distinct` distinct labels (negative ones among them), shuffled.
    pattern: "tie" three labels share the maximum 3, anywhere; "late" one label first seen after the 48th holds the unique
    maximum; "late_tie" three labels share the maximum, the last-seen label among them"""
    values = rng.choice(np.arange(-40, 400), size=distinct, replace=False)
    if not (values < 0).any():
        values[0] = -7 if -7 not in values else -8
    counts = rng.integers(1, 3, size=distinct)
    if pattern == "tie":
        counts[rng.choice(distinct, size=3, replace=False)] = 3
        seq = np.repeat(values, counts)
        return seq[rng.permutation(len(seq))]
    first = values[rng.permutation(distinct)]                          # first-seen order
    rest_counts = np.ones(distinct, np.int64)
    if pattern == "late":
        assert distinct > MAXL
        rest_counts[:MAXL] += rng.integers(0, 3, size=MAXL)             # at most 4 of each of the first 48
        rest_counts[distinct - 1 if distinct < MAXL + 6 else distinct - 5] = 5
    else:
        rest_counts[[3, distinct - 1, distinct - 4]] = 3
    rest = np.repeat(first, rest_counts)
    return np.concatenate([first, rest[rng.permutation(len(rest))]])


def _label_set(name, sizes, patterns, copies):
    rng = _rng(name)
    pts, labs, want = [], [], []
    cell = 0
    for d in sizes:
        for pattern in patterns:
            for _ in range(copies):
                seq = _label_cell(rng, d, pattern)
                corner = np.asarray([cell % 5, (cell // 5) % 5, cell // 25], np.float64)
                pts.append((corner + rng.uniform(0.1, 0.9, size=(len(seq), 3))) * 0.5)
                labs.append(seq)
                want.append((d, pattern))
                cell += 1
    n = [len(a) for a in pts]
    # interleave the cells without disturbing the order inside one cell
    owner = np.repeat(np.arange(len(n)), n)
    owner = owner[rng.permutation(len(owner))]
    cursor = np.zeros(len(n), np.int64)
    p, c = np.zeros((len(owner), 3)), np.zeros(len(owner), np.int32)
    for i, o in enumerate(owner):
        p[i], c[i] = pts[o][cursor[o]], labs[o][cursor[o]]
        cursor[o] += 1
    return p, c, want


def labels_many():
    p, c, want = _label_set("labels_many", LABEL_CELL_SIZES, ("tie",), 3)
    c2 = np.stack([c, 1000 - 3 * c], 1)                                # the same histograms under other labels: other buckets
    return _data(p, [len(p)], 0.5, c=c2, cells=want)


def labels_overflow():
    p, c, want = _label_set("labels_overflow", OVERFLOW_CELL_SIZES, ("late", "late_tie", "tie"), 1)
    return _data(p, [len(p)], 0.5, c=c, cells=want)


def emit():
    rng = _rng("emit")
    parts = [lattice_points(rng, m, 6, LATTICE_DL, (0.0, LATTICE_DL * 40 * b, 0.0)) for b, m in enumerate(EMIT_M)]
    p = np.concatenate(parts)
    f = rng.normal(size=(len(p), max(EMIT_FD))) * 10
    c = np.stack([rng.integers(0, 4, size=len(p)), rng.integers(-2, 6, size=len(p)), rng.integers(0, 2, size=len(p))], 1)
    return _data(p, [len(a) for a in parts], LATTICE_DL, f=f, c=c, m=list(EMIT_M))


def scan(n):
    rng = _rng("scan", n)
    return _data(rng.uniform(-3, 3, size=(n, 3)), [n], 0.7)


def scan_small():
    rng = _rng("scan_small")
    return _data(rng.uniform(-1, 1, size=(66, 3)), [32, 33, 1], 0.4)


def reuse_calls():
    """the three calls of the workspace-reuse test: 10 000 points in two elements; 40 points in five; features and labels"""
    rng = _rng("reuse")
    big = _data(rng.uniform(-4, 4, size=(10000, 3)), [6000, 4000], 0.4)
    small = _data(rng.uniform(-1, 1, size=(40, 3)), [7, 0, 20, 12, 1], 0.3)
    e = emit()
    return [big, small, _data(e["p"], e["lens"], e["dl"], f=e["f"][:, :3], c=e["c"][:, :2])]


_BUILDERS = {"wrapped_key": wrapped_key, "crowded": crowded, "labels_many": labels_many, "labels_overflow": labels_overflow,
             "emit": emit, "mixed": mixed, "scan_small": scan_small}
_SETS = {}


def dataset(name):
    if name not in _SETS:
        if name in _BUILDERS:
            _SETS[name] = _BUILDERS[name]()
        elif name.startswith("lattice"):
            _SETS[name] = lattice(int(name[7:]))
        elif name.startswith("rounding"):
            _SETS[name] = rounding(float(name[8:]))
        elif name.startswith("scan"):
            _SETS[name] = scan(int(name[4:]))
        else:
            raise KeyError(name)
    return _SETS[name]


LATTICE_SETS = ["lattice%d" % m for m in ROW_COUNTS]
ROUNDING_SETS = ["rounding%g" % dl for dl in ROUNDING_DLS]
SCAN_SETS = ["scan%d" % n for n in SCAN_N] + ["scan_small"]
ALL_SETS = LATTICE_SETS + ["mixed"] + ROUNDING_SETS + ["wrapped_key", "crowded", "labels_many", "labels_overflow", "emit"] + SCAN_SETS
