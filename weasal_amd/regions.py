"""The per-sphere regions of the weak-label sampler on the device: from the spheres of a batch (weasal_amd.sampler) and the
anchors of their tiles (weasal_amd.anchors.AnchorSet) to `batch.region` / `batch.region_lb` as CSR device tensors, and the
region means the overlap-region loss takes of the class-activation maps (csrc/regions.hip).

Reference: datasets/DALES_WeakLabel.py:424-451 (identical in Vaihingen3D_WeakLabel.py:418-445).  There every sphere makes one
KD-tree query on the anchor centres and, per candidate anchor, an np.in1d, an argsort and a searchsorted against the sphere's
`input_inds`, in a Python loop on the host.  Here a batch is cut by count, ONE host read, fill (the pattern of
anchors.anchors_with_points): the read brings the number of regions, the number of their rows and the status word; nothing of
size N, nnz or A leaves the device.

Contract (include/weasal_hip.h):
  * candidates of a sphere: the anchors of its tile with d2 = (dx*dx + dy*dy) + dz*dz <= r*r in float64, every product and sum
    rounded, r = in_radius - sub_radius - 0.01 evaluated on the host in float64 as written (:434);
  * the region of (sphere, anchor): the members of the anchor that occur in the sphere's slice of `input_inds` (ascending tile
    point ids), each replaced by its position in that slice;
  * a region is dropped when it is empty or holds local row 0 alone (`if idx.any()`, :449, on OUR order of input_inds);
  * kept regions are ordered by sphere, then by ascending anchor id; an anchor listed twice in its set gives two regions.
"""
import numpy as np
import torch

from . import _lib, ops
from ._lib import check, current_stream, ptr
from .active import MAX_CLASSES

MAX_SPHERES = 64                 # WS_REGION_MAX_SPHERES (sampler.MAX_SPHERES)
_WORDS = 3                       # WS_REGION_WORDS: regions, their rows, labels outside [0, n_class)


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


class SphereRegions:
    """The regions of one batch.  Device tensors: ptr int64 [R + 1] and idx int64 [nnz] (CSR; idx = rows of the stacked batch,
    ascending inside a region), reg int32 [nnz] (the region of every entry of idx), sphere int32 [R], anchor int64 [R] (the id
    in the tile's AnchorSet), lb float32 [R, C] (0/1 label rows), inv_len float32 [R] (1 / length), the transpose t_ptr int64
    [N + 1] / t_reg int32 [nnz] (the regions of every row, ascending), cloud_lb float32 [B, C] (column k = 1 iff a row of the
    sphere has label k, :474-476).  Host: lengths int64 [B], n_regions, nnz.  The sphere-local row of an entry is
    idx - row_off[sphere] (row_off: the exclusive sum of lengths); to_lists() spells it out."""

    def __init__(self, ptr, idx, reg, sphere, anchor, lb, inv_len, t_ptr, t_reg, cloud_lb, lengths, n_regions, nnz):
        self.ptr, self.idx, self.reg, self.sphere, self.anchor, self.lb, self.inv_len = ptr, idx, reg, sphere, anchor, lb, inv_len
        self.t_ptr, self.t_reg, self.cloud_lb = t_ptr, t_reg, cloud_lb
        self.lengths = np.asarray(lengths, np.int64).reshape(-1)
        self.n_regions, self.nnz = int(n_regions), int(nnz)

    def __len__(self):
        return self.n_regions

    @property
    def n_rows(self):
        return int(self.lengths.sum())

    def to_lists(self):
        """-> (region, region_lb) in the reference's layout: region[s] = list of int64 arrays of sphere-local rows,
        region_lb[s] = list of float32 [C] rows (what `batch.region` / `batch.region_lb` hold on the list path).  Reads the
        tensors back: for the CPU oracle, the list path and the tests."""
        ptr_h, idx_h, sph_h, lb_h = _host(self.ptr), _host(self.idx), _host(self.sphere), _host(self.lb)
        row_off = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        region = [[] for _ in range(self.lengths.shape[0])]
        region_lb = [[] for _ in range(self.lengths.shape[0])]
        for r in range(self.n_regions):
            s = int(sph_h[r])
            region[s].append(idx_h[ptr_h[r]:ptr_h[r + 1]].astype(np.int64) - row_off[s])
            region_lb[s].append(lb_h[r].astype(np.float32))
        return region, region_lb


def prepare(anchor_set):
    """keep a device copy of the set's float64 centres with it, so that they are uploaded once per tile and not per batch
    -> that copy ([A, 3] float64)"""
    d = getattr(anchor_set, "centres_dev", None)
    if d is None or d.shape[0] != len(anchor_set):
        c = np.ascontiguousarray(np.asarray(anchor_set.centres, np.float64).reshape(-1, 3))
        d = torch.from_numpy(c).to(anchor_set.ptr.device)
        anchor_set.centres_dev = d
    return d


def search_radius(in_radius, sub_radius):
    """`self.config.in_radius-self.config.sub_radius-0.01` (:434) in float64"""
    return float(in_radius) - float(sub_radius) - 0.01


def cut_regions(anchor_sets, cloud_inds, centres, input_inds, lengths, labels, in_radius, sub_radius, n_class):
    """-> SphereRegions of one batch of the sampler.  anchor_sets: one AnchorSet per tile (an empty one where a tile has no
    anchors); cloud_inds [B] (host: the tile of every sphere) and centres [B, 3] (host float64: SphereSampler.last_centres);
    input_inds [N] int64 and labels [N] (device: the sampler's outputs, labels already mapped to [0, n_class)); lengths [B]
    (host).  A label outside [0, n_class) raises ValueError after the one read."""
    lib = _lib.lib()
    ops._need_cuda(input_inds, labels)
    n_class = int(n_class)
    if n_class < 1 or n_class > MAX_CLASSES:
        raise ValueError("n_class = %d (1 to %d classes)" % (n_class, MAX_CLASSES))
    lens = np.asarray(lengths, np.int64).reshape(-1)
    tiles = np.asarray(cloud_inds, np.int64).reshape(-1)
    cen = np.ascontiguousarray(np.asarray(centres, np.float64).reshape(-1, 3))
    nb = lens.shape[0]
    if not 1 <= nb <= MAX_SPHERES:
        raise ValueError("a batch holds 1 to %d spheres (got %d)" % (MAX_SPHERES, nb))
    if tiles.shape[0] != nb or cen.shape[0] != nb or (lens < 0).any():
        raise ValueError("cloud_inds, centres and lengths must hold one entry per sphere")
    if tiles.min() < 0 or tiles.max() >= len(anchor_sets):
        raise ValueError("cloud_inds outside [0, %d)" % len(anchor_sets))
    row_off = np.zeros(nb + 1, np.int64)
    np.cumsum(lens, out=row_off[1:])
    n = int(row_off[-1])
    inds = input_inds.detach().reshape(-1).to(torch.int64).contiguous()
    lab = labels.detach().reshape(-1).to(torch.int64).contiguous()
    if inds.shape[0] != n or lab.shape[0] != n:
        raise ValueError("input_inds and labels must hold sum(lengths) = %d rows" % n)
    dev = inds.device
    pair_off = np.zeros(nb + 1, np.int64)
    np.cumsum([len(anchor_sets[t]) for t in tiles], out=pair_off[1:])
    pairs = int(pair_off[-1])
    if pairs >= 2 ** 31:
        raise ValueError("%d (sphere, anchor) pairs in one batch (below 2^31)" % pairs)
    order = np.argsort(tiles, kind='stable').astype(np.int32)                  # the spheres grouped by tile
    # one upload: row_off, pair_off, the centres' bits, the grouped sphere ids
    table = np.concatenate([row_off, pair_off, cen.reshape(-1).view(np.int64),
                            np.concatenate([order, np.zeros(nb % 2, np.int32)]).view(np.int64)])
    d_table = torch.from_numpy(table).to(dev)
    d_row_off, d_pair_off = d_table[:nb + 1], d_table[nb + 1:2 * (nb + 1)]
    d_cen = d_table[2 * (nb + 1):2 * (nb + 1) + 3 * nb].view(torch.float64)
    d_order = d_table[2 * (nb + 1) + 3 * nb:].view(torch.int32)
    groups = []                                                               # (tile, first position in d_order, spheres)
    for pos in range(nb):
        t = int(tiles[order[pos]])
        if groups and groups[-1][0] == t:
            groups[-1][2] += 1
        else:
            groups.append([t, pos, 1])
    groups = [g for g in groups if len(anchor_sets[g[0]]) > 0]
    radius = search_radius(in_radius, sub_radius)
    if not radius >= 0.0:
        groups = []                                                           # (no anchor can be a candidate)
    work = torch.zeros(3 * (pairs + 1), dtype=torch.int32, device=dev)
    cnt, slot, ptr32 = work[:pairs + 1], work[pairs + 1:2 * (pairs + 1)], work[2 * (pairs + 1):]
    words = torch.empty(_WORDS, dtype=torch.int64, device=dev)
    cloud_lb = torch.empty((nb, n_class), dtype=torch.float32, device=dev)
    scratch = torch.empty(lib.ws_region_scratch_bytes(pairs), dtype=torch.uint8, device=dev)
    st = current_stream()
    for t, pos, ng in groups:
        a = anchor_sets[t]
        ops._need_cuda(a.ptr, a.idx, a.bits)
        check(lib.ws_region_cut_count(ptr(prepare(a)), ptr(a.ptr), ptr(a.idx), a.idx.shape[0], len(a), ptr(d_order[pos:]), ng, nb,
                                      ptr(d_cen), ptr(d_row_off), ptr(d_pair_off), ptr(inds), n, pairs, radius, ptr(cnt), st))
    check(lib.ws_region_cut_scan(ptr(cnt), pairs, ptr(slot), ptr(ptr32), ptr(lab), ptr(d_row_off), n, nb, n_class, ptr(cloud_lb),
                                 ptr(words), ptr(scratch), st))
    host = words.cpu().numpy()                                                 # the one read between count and fill
    if int(host[2]) != 0:
        raise ValueError("regions: labels holds %d values outside [0, n_class) (skipped on the device)" % int(host[2]))
    n_reg, nnz = int(host[0]), int(host[1])
    o_ptr = torch.empty(n_reg + 1, dtype=torch.int64, device=dev)
    o_ptr[n_reg:].fill_(nnz)
    o_idx = torch.empty(nnz, dtype=torch.int64, device=dev)
    o_reg = torch.empty(nnz, dtype=torch.int32, device=dev)
    o_sphere = torch.empty(n_reg, dtype=torch.int32, device=dev)
    o_anchor = torch.empty(n_reg, dtype=torch.int64, device=dev)
    o_lb = torch.empty((n_reg, n_class), dtype=torch.float32, device=dev)
    o_inv = torch.empty(n_reg, dtype=torch.float32, device=dev)
    if n_reg > 0:
        for t, pos, ng in groups:
            a = anchor_sets[t]
            check(lib.ws_region_cut_fill(ptr(a.ptr), ptr(a.idx), a.idx.shape[0], ptr(a.bits), len(a), ptr(d_order[pos:]), ng, nb,
                                         ptr(d_row_off), ptr(d_pair_off), ptr(inds), n, pairs, ptr(cnt), ptr(slot), ptr(ptr32), n_reg,
                                         nnz, n_class, ptr(o_ptr), ptr(o_idx), ptr(o_reg), ptr(o_sphere), ptr(o_anchor), ptr(o_lb),
                                         ptr(o_inv), st))
    # the transpose point -> regions: the entries are in (region, row) order, so a stable sort by row leaves the regions of a
    # row ascending; t_ptr[p] = the entries whose row is below p
    sorted_idx, perm = torch.sort(o_idx, stable=True)
    t_reg = o_reg[perm]
    t_ptr = torch.searchsorted(sorted_idx, torch.arange(n + 1, dtype=torch.int64, device=dev))
    return SphereRegions(o_ptr, o_idx, o_reg, o_sphere, o_anchor, o_lb, o_inv, t_ptr, t_reg, cloud_lb, lens, n_reg, nnz)
