"""Weak-label anchors of a tile on the device: from the resident points and sub labels to the CSR lists and 0/1 label rows
that stage 2 (refine) and stage 3 (active) start from (csrc/anchors.hip).

Reference: utils/anchors.py, driven per tile by datasets/DALES_WeakLabel.py:201-269.  There the members of every anchor
come from one KD-tree query and one np.unique per anchor in a Python loop (:83-99), the overlaps from one np.in1d per
neighbouring pair (:119-139), and both live in pickled dictionaries.  Here the points and labels are the device tensors the
SphereSampler already holds; the anchors become CSR device tensors (`ptr`, `idx`: int64) with one uint32 of label bits per
anchor, and the host keeps what is of size A only: centres, label rows, `kept`.

Arithmetic contract (weasal_hip.h): a float32 coordinate widened to float64, d2 = (dx*dx + dy*dy) + dz*dz with every
product and sum rounded, inside iff d2 <= radius*radius.  Lists are ascending.  New overlap anchors follow the A inputs in
(i, j) lexicographic order of their pair (the reference's own order follows its tree traversal and is unspecified), and
are never paired themselves.  Everything but the centres of the new anchors is exact and the same on every run; a centre is
the float64 mean of its members.

Host reads: get_anchors six floats; anchors_with_points the two totals between count and fill, then the A label words
and `kept`; update_anchors the number of candidate pairs, the totals between count and fill, then the new anchors' words and
centres.  Nothing of size N or nnz leaves the device.
"""
import random

import numpy as np
import torch

from . import _lib, ops
from ._lib import check, current_stream, ptr
from .active import MAX_CLASSES, _host_ids

STATUS_WORDS = 2
TOTAL_WORDS = 3
_STATUS_NAMES = ("labels holds %d values outside [0, n_class)",
                 "use_anchors holds %d anchor ids outside [0, A)")
_MAX_CELLS = 1 << 22
_CELL_MARGIN = 1.0 + 2.0 ** -20         # cell > radius, so that rounding in floor((v - o) / cell) cannot lose a neighbour


def unpack_label_bits(bits, n_class):
    """uint32 [A] -> host int [A, n_class] of zeros and ones, column k = bit k (the inverse of refine.pack_label_rows)"""
    b = np.asarray(bits, dtype=np.uint32).reshape(-1, 1)
    return ((b >> np.arange(n_class, dtype=np.uint32)) & np.uint32(1)).astype(np.int64)


class AnchorSet:
    """The anchors of one tile.  centres float64 [A, 3] (host), ptr int64 [A + 1] and idx int64 [nnz] (device CSR,
    ascending inside an anchor), bits uint32 [A] (device), lb int [A, n_class] (host 0/1 rows, unpacked from bits), kept
    int64 [n_base] (host: the index of each base anchor among the anchors handed to anchors_with_points; -1 for an
    overlap anchor that a later selection made a base anchor), n_base: the number of anchors before the overlap anchors were appended.

    ptr, idx and lb go as they are into refine.refine_cloud / weak_label_mask and active.select_anchors / anchor_scores."""

    def __init__(self, centres, ptr, idx, bits, lb, kept, n_base):
        self.centres, self.ptr, self.idx, self.bits, self.lb, self.kept, self.n_base = centres, ptr, idx, bits, lb, kept, int(n_base)

    def __len__(self):
        return int(self.lb.shape[0])

    @property
    def n_class(self):
        return int(self.lb.shape[1])

    def save(self, path):
        """a plain .npz of the arrays (np.savez appends '.npz' to a path without it)"""
        np.savez(path, centres=self.centres, ptr=self.ptr.cpu().numpy(), idx=self.idx.cpu().numpy(),
                 bits=self.bits.cpu().numpy(), lb=self.lb, kept=self.kept, n_base=np.int64(self.n_base))

    @classmethod
    def load(cls, path, device):
        with np.load(path, allow_pickle=False) as z:
            return cls(z["centres"], torch.from_numpy(z["ptr"]).to(device), torch.from_numpy(z["idx"]).to(device),
                       torch.from_numpy(z["bits"]).to(device), z["lb"], z["kept"], int(z["n_base"]))


def _raise_on_status(words):
    bad = [msg % int(v) for msg, v in zip(_STATUS_NAMES, words) if int(v) != 0]
    if bad:
        raise ValueError("anchors: " + "; ".join(bad) + " (skipped on the device)")


def _linspace(start, stop, num):
    """np.linspace(start, stop, num) for float64 scalars, spelled out: arange(num) * ((stop - start) / (num - 1)) + start
    with the last entry set to stop"""
    start, stop = np.float64(start), np.float64(stop)
    if num == 1:
        return np.array([start], np.float64)
    div = np.float64(num - 1)
    delta = stop - start
    y = np.arange(num, dtype=np.float64)
    step = delta / div
    y = y * step if step != 0 else (y / div) * delta
    y = y + start
    y[-1] = stop
    return y


def anchors_from_bounds(bounds, sub_radius, method='full'):
    """the host part of get_anchors: bounds = float32 (x min, x max, y min, y max, z min, z max)"""
    if method == 'full':
        spacing = np.float64(sub_radius)
    elif method == 'reduced':
        spacing = np.float64(2 * sub_radius)
    else:
        raise ValueError('Unsupported method (' + method + ') for creating anchor points')
    b = np.asarray(bounds, dtype=np.float32).reshape(3, 2)
    axes = []
    for lo, hi in b:
        extent = np.float64(np.float32(hi - lo))                               # the float32 difference, then widened
        num = int(np.floor(extent / spacing) + 1)
        axes.append(_linspace(lo, hi, num))
    x, y, z = np.meshgrid(*axes, indexing='ij')                                # nested loops x, y, z: z runs fastest
    base = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1)
    if method == 'full':
        return base
    r = np.float64(sub_radius)
    shifts = np.array([[0, 0, 0], [0, 0, 1], [1, 1, 0], [1, 1, 1]], np.float64) * r
    return (base[:, None, :] + shifts[None, :, :]).reshape(-1, 3)


def cloud_bounds(points):
    """-> host float32 [6] (x min, x max, y min, y max, z min, z max) of device points [N, 3]: one kernel chain, one read"""
    lib = _lib.lib()
    ops._need_cuda(points)
    p = ops._f32c(points)
    if p.dim() != 2 or p.shape[1] != 3 or p.shape[0] < 1:
        raise ValueError("points must be [N, 3] with N >= 1")
    out = torch.empty(6, dtype=torch.float32, device=p.device)
    check(lib.ws_anchor_bounds(ptr(p), p.shape[0], ptr(out), current_stream()))
    return out.cpu().numpy()


def get_anchors(points, sub_radius, method='full'):
    """-> host float64 [A0, 3]: the regular anchor positions of utils/anchors.py:26-73 for device points [N, 3] float32.
    'full': spacing sub_radius; 'reduced': spacing 2 * sub_radius and four shifted copies per lattice point."""
    if method not in ('full', 'reduced'):
        raise ValueError('Unsupported method (' + method + ') for creating anchor points')
    return anchors_from_bounds(cloud_bounds(points), sub_radius, method)


def _grid(centres, reach):
    """uniform grid over host centres [M, 3] float64 with cell > reach: (h_grid float64 [7], cell_start int32, cell_item
    int32); z is the fastest axis and the items of a cell are ascending"""
    c = np.asarray(centres, np.float64)
    origin = c.min(axis=0)
    span = c.max(axis=0) - origin
    cell = float(reach) * _CELL_MARGIN
    if not np.isfinite(span).all() or not np.isfinite(cell) or cell < 0:
        raise ValueError("anchor centres and radius must be finite")
    floor = float(span.max()) / 128.0                                          # at most 129 cells per axis: 2.1 M in all
    with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
        many = cell <= 0 or not np.prod(np.floor(span / cell) + 1) <= _MAX_CELLS
    if many:
        cell = max(cell, floor) if floor > 0 else 1.0
    dims = np.floor(span / cell).astype(np.int64) + 1
    ijk = np.minimum(np.floor((c - origin) / cell).astype(np.int64), dims - 1)
    key = (ijk[:, 0] * dims[1] + ijk[:, 1]) * dims[2] + ijk[:, 2]
    order = np.argsort(key, kind='stable')
    start = np.zeros(int(dims.prod()) + 1, np.int64)
    np.cumsum(np.bincount(key, minlength=int(dims.prod())), out=start[1:])
    h_grid = np.array([origin[0], origin[1], origin[2], cell, dims[0], dims[1], dims[2]], np.float64)
    return h_grid, start.astype(np.int32), order.astype(np.int32)


def _host_ptr(a):
    import ctypes
    return ctypes.c_void_p(a.ctypes.data)


def _kept_all(anchor_set):
    """`kept` with one entry per anchor of the set: an overlap anchor has no original index, -1"""
    extra = len(anchor_set) - anchor_set.kept.shape[0]
    return np.concatenate([anchor_set.kept, np.full(extra, -1, np.int64)])


def _empty_set(n_class, device):
    return AnchorSet(np.zeros((0, 3), np.float64), torch.zeros(1, dtype=torch.int64, device=device),
                     torch.zeros(0, dtype=torch.int64, device=device), torch.zeros(0, dtype=torch.uint32, device=device),
                     np.zeros((0, n_class), np.int64), np.zeros(0, np.int64), 0)


def anchors_with_points(points, labels, anchors, radius, n_class):
    """-> AnchorSet of the anchors that have points inside (utils/anchors.py:75-103).  points [N, 3] float32 and labels
    [N] (int) on the device, anchors host float64 [A0, 3] (get_anchors), radius the sub_radius.  Anchors without members
    are dropped, the others keep their order (`kept`).  A label outside [0, n_class) raises ValueError."""
    lib = _lib.lib()
    ops._need_cuda(points, labels)
    n_class = int(n_class)
    if n_class < 1 or n_class > MAX_CLASSES:
        raise ValueError("n_class = %d (1 to %d classes)" % (n_class, MAX_CLASSES))
    p = ops._f32c(points)
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError("points must be [N, 3]")
    n = p.shape[0]
    lab = labels.detach().reshape(-1).to(torch.int32).contiguous()
    if lab.shape[0] != n:
        raise ValueError("labels must hold one entry per point")
    anc = np.ascontiguousarray(np.asarray(anchors, np.float64).reshape(-1, 3))
    a0 = anc.shape[0]
    dev = p.device
    if a0 == 0:
        return _empty_set(n_class, dev)
    radius = float(radius)
    h_grid, cell_start, cell_item = _grid(anc, radius)
    d_anc = torch.from_numpy(anc).to(dev)
    d_start = torch.from_numpy(cell_start).to(dev)
    d_item = torch.from_numpy(cell_item).to(dev)
    work = torch.empty(3 * (a0 + 1) + a0, dtype=torch.int32, device=dev)       # counts, slot, ptr32 [a0 + 1] each; cursor [a0]
    counts, slot, ptr32 = work[:a0 + 1], work[a0 + 1:2 * (a0 + 1)], work[2 * (a0 + 1):3 * (a0 + 1)]
    cursor = work[3 * (a0 + 1):]
    bits0 = torch.empty(a0, dtype=torch.uint32, device=dev)
    words = torch.zeros(TOTAL_WORDS + STATUS_WORDS, dtype=torch.int64, device=dev)
    totals, status = words[:TOTAL_WORDS], words[TOTAL_WORDS:]
    scratch = torch.empty(lib.ws_anchor_scratch_bytes(a0), dtype=torch.uint8, device=dev)
    st = current_stream()
    check(lib.ws_anchor_members_plan(ptr(p), ptr(lab), n, n_class, ptr(d_anc), a0, radius, _host_ptr(h_grid), ptr(d_start),
                                     ptr(d_item), ptr(counts), ptr(slot), ptr(ptr32), ptr(bits0), ptr(totals), ptr(status),
                                     ptr(scratch), st))
    host = words.cpu().numpy()                                                 # the one read between count and fill
    _raise_on_status(host[TOTAL_WORDS:])
    n_kept, nnz = int(host[0]), int(host[1])
    kept = torch.empty(n_kept, dtype=torch.int64, device=dev)
    a_ptr = torch.empty(n_kept + 1, dtype=torch.int64, device=dev)
    a_idx = torch.empty(nnz, dtype=torch.int64, device=dev)
    centres = torch.empty((n_kept, 3), dtype=torch.float64, device=dev)
    bits = torch.empty(n_kept, dtype=torch.uint32, device=dev)
    check(lib.ws_anchor_members_fill(ptr(p), n, ptr(d_anc), a0, radius, _host_ptr(h_grid), ptr(d_start), ptr(d_item), ptr(counts),
                                     ptr(slot), ptr(ptr32), ptr(bits0), n_kept, nnz, ptr(kept), ptr(a_ptr), ptr(a_idx), ptr(centres),
                                     ptr(bits), ptr(cursor), st))
    kept_h = kept.cpu().numpy()
    return AnchorSet(anc[kept_h], a_ptr, a_idx, bits, unpack_label_bits(bits.cpu().numpy(), n_class), kept_h, n_kept)


def update_anchors(anchor_set, points, sub_radius, use_anchors=None):
    """-> AnchorSet: the anchors of `anchor_set` (all of them, or those listed in use_anchors, in that order, repeats
    allowed: select_anchors of DALES_WeakLabel.py:241-263) followed by one new anchor per neighbouring pair whose label
    rows differ and whose point lists intersect (utils/anchors.py:105-143).  points: the device points the set was built
    from.  An entry of use_anchors outside [0, A) raises ValueError before the device is touched."""
    lib = _lib.lib()
    ops._need_cuda(points, anchor_set.ptr, anchor_set.idx, anchor_set.bits)
    p = ops._f32c(points)
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError("points must be [N, 3]")
    dev = p.device
    na = len(anchor_set)
    n_class = anchor_set.n_class
    if use_anchors is None:
        sel_h, sel, ns = None, None, na
        base_centres = anchor_set.centres
    else:
        sel_h = _host_ids(use_anchors)
        bad = int(((sel_h < 0) | (sel_h >= na)).sum())
        if bad:
            _raise_on_status([0, bad])
        ns = sel_h.shape[0]
        base_centres = anchor_set.centres[sel_h]
    if ns == 0:
        return _empty_set(n_class, dev)
    reach = 1.5 * float(sub_radius)                                            # :115
    h_grid, cell_start, cell_item = _grid(base_centres, reach)
    if sel_h is not None:
        sel = torch.from_numpy(sel_h).to(dev)
    d_centres = torch.from_numpy(np.ascontiguousarray(anchor_set.centres, np.float64)).to(dev)
    d_start = torch.from_numpy(cell_start).to(dev)
    d_item = torch.from_numpy(cell_item).to(dev)
    a_ptr, a_idx, a_bits = anchor_set.ptr, anchor_set.idx, anchor_set.bits
    nnz = a_idx.shape[0]
    words = torch.zeros(TOTAL_WORDS + STATUS_WORDS, dtype=torch.int64, device=dev)
    totals, status = words[:TOTAL_WORDS], words[TOTAL_WORDS:]
    st = current_stream()
    # the candidate pairs
    pair_work = torch.empty(2 * (ns + 1), dtype=torch.int32, device=dev)
    pair_cnt, pair_ptr = pair_work[:ns + 1], pair_work[ns + 1:]
    scratch = torch.empty(lib.ws_anchor_scratch_bytes(ns), dtype=torch.uint8, device=dev)
    check(lib.ws_anchor_pairs_plan(ptr(d_centres), na, ptr(sel), ns, reach, _host_ptr(h_grid), ptr(d_start), ptr(d_item),
                                   ptr(pair_cnt), ptr(pair_ptr), ptr(totals), ptr(status), ptr(scratch), st))
    host = words.cpu().numpy()
    _raise_on_status(host[TOTAL_WORDS:])
    n_pairs = int(host[0])
    pairs = torch.empty(2 * max(n_pairs, 1), dtype=torch.int32, device=dev)
    pair_i, pair_j = pairs[:max(n_pairs, 1)], pairs[max(n_pairs, 1):]
    check(lib.ws_anchor_pairs_fill(ptr(d_centres), na, ptr(sel), ns, reach, _host_ptr(h_grid), ptr(d_start), ptr(d_item),
                                   ptr(pair_ptr), n_pairs, ptr(pair_i), ptr(pair_j), st))
    # count, one read, fill
    ov = torch.empty(3 * (n_pairs + 1) + ns + 1, dtype=torch.int32, device=dev)
    inter_cnt, new_slot = ov[:n_pairs + 1], ov[n_pairs + 1:2 * (n_pairs + 1)]
    new_ptr, sel_ptr = ov[2 * (n_pairs + 1):3 * (n_pairs + 1)], ov[3 * (n_pairs + 1):]
    scratch = torch.empty(lib.ws_anchor_scratch_bytes(max(n_pairs, ns)), dtype=torch.uint8, device=dev)
    check(lib.ws_anchor_overlap_plan(ptr(a_ptr), ptr(a_idx), nnz, ptr(a_bits), na, ptr(sel), ns, ptr(pair_i), ptr(pair_j), n_pairs,
                                     ptr(inter_cnt), ptr(new_slot), ptr(new_ptr), ptr(sel_ptr), ptr(totals), ptr(scratch), st))
    n_new, nnz_new, nnz_sel = (int(v) for v in totals.cpu().numpy())
    rows = ns + n_new
    o_ptr = torch.empty(rows + 1, dtype=torch.int64, device=dev)
    o_idx = torch.empty(nnz_sel + nnz_new, dtype=torch.int64, device=dev)
    o_bits = torch.empty(rows, dtype=torch.uint32, device=dev)
    o_centres = torch.empty((rows, 3), dtype=torch.float64, device=dev)
    check(lib.ws_anchor_overlap_fill(ptr(p), p.shape[0], ptr(a_ptr), ptr(a_idx), nnz, ptr(a_bits), ptr(d_centres), na, ptr(sel), ns,
                                     ptr(pair_i), ptr(pair_j), n_pairs, ptr(inter_cnt), ptr(new_slot), ptr(new_ptr), ptr(sel_ptr),
                                     n_new, nnz_new, nnz_sel, ptr(o_ptr), ptr(o_idx), ptr(o_bits), ptr(o_centres), st))
    centres = np.concatenate([np.asarray(base_centres, np.float64), o_centres[ns:].cpu().numpy()])
    kept = _kept_all(anchor_set) if sel_h is None else _kept_all(anchor_set)[sel_h]
    return AnchorSet(centres, o_ptr, o_idx, o_bits, unpack_label_bits(o_bits.cpu().numpy(), n_class), kept, ns)


# ----------------------------------------------------------------------------------------------------------------------
# host-only parts: they work on the [A, C] label rows
# ----------------------------------------------------------------------------------------------------------------------
def _regular(count, picks):
    """`picks` indices spread evenly over range(count): round(linspace(0, count - 1, picks))"""
    return np.round(np.linspace(0, count - 1, picks)).astype(int)


def subsample_indices(anchor_lb, anchor_count, subsample_method, n_anchors=None):
    """-> sorted list of anchor ids (`anchor_inds_sub` of utils/anchors.py:162-262) for host label rows [A, C].
    'regular': evenly spaced; 'random': random.choices, with replacement; 'balanced': up to four rounds that give every
    class the same share of what is still missing, then random.choices from the rest.  The draws come from Python's
    `random`, so random.seed fixes them as it does in the reference."""
    lb = np.asarray(anchor_lb)
    total = len(lb)
    if anchor_count > total:
        raise ValueError('Selected anchor count (' + str(anchor_count) + ') exceeds the number of anchors (' + str(total) + ')!')
    if subsample_method == 'regular':
        return _regular(total if n_anchors is None else n_anchors, anchor_count)
    if subsample_method == 'random':
        return sorted(random.choices(list(range(total)), k=anchor_count))
    if subsample_method != 'balanced':
        raise ValueError('Subsample method "' + subsample_method + '" is not supported!')
    n_class = lb.shape[1]
    pool = list(range(total))
    chosen = []
    missing = anchor_count
    for _ in range(4):
        share = int(missing / n_class)
        rows = lb[pool] == 1 if pool else np.zeros((0, n_class), bool)
        picked = set()
        for k in range(n_class):
            holders = [pool[i] for i in np.nonzero(rows[:, k])[0]]
            if len(holders) >= share:
                picked.update(holders[i] for i in _regular(len(holders), share))
            else:
                picked.update(holders)
        chosen += sorted(picked)
        pool = [a for a in pool if a not in picked]
        missing = anchor_count - len(chosen)
        if missing < n_class:
            break
    chosen += random.choices(pool, k=missing)
    return sorted(chosen)


def select_anchors(anchor_set, anchor_inds_sub):
    """-> AnchorSet holding the listed anchors, in that order, repeats allowed (utils/anchors.py:145-160)"""
    sel = _host_ids(anchor_inds_sub)
    na = len(anchor_set)
    bad = int(((sel < 0) | (sel >= na)).sum())
    if bad:
        _raise_on_status([0, bad])
    dev = anchor_set.ptr.device
    d_sel = torch.from_numpy(sel).to(dev)
    beg = anchor_set.ptr[d_sel]
    lens = anchor_set.ptr[d_sel + 1] - beg
    o_ptr = torch.zeros(sel.shape[0] + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=o_ptr[1:])
    row = torch.repeat_interleave(torch.arange(sel.shape[0], device=dev), lens)
    o_idx = anchor_set.idx[beg[row] + torch.arange(row.shape[0], device=dev) - o_ptr[row]]
    bits = anchor_set.bits.view(torch.int32)[d_sel].view(torch.uint32)
    return AnchorSet(anchor_set.centres[sel], o_ptr, o_idx, bits, anchor_set.lb[sel], _kept_all(anchor_set)[sel], sel.shape[0])


def subsample_anchors(anchor_set, anchor_count, subsample_method):
    """-> (AnchorSet, anchor_inds_sub): utils/anchors.py:162-268"""
    inds = subsample_indices(anchor_set.lb, anchor_count, subsample_method, n_anchors=anchor_set.centres.shape[0])
    return select_anchors(anchor_set, inds), inds
