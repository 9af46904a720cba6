"""Pseudo-label refinement on the device: from the weak-label votes of a pass over the training tiles to the pseudo labels
and class weights that the stage-3 training reads (csrc/refine.hip).

Reference: pseudoLabel_refinement.py.  Per tile (:63-68) every point gets the product of the 0/1 label rows of the anchors
that list it; (:123-145) a point whose largest vote among the classes its weak labels allow falls below `threshold` percent
becomes the uncertain label 10, every other point keeps the arg-max label of its votes; (:148-151) the labels are counted
by value over all tiles; (:168-169) the counts become the class weights of the stage-3 loss.  The reference does this on
the host with a KD-tree, a Python loop over the anchor dictionary and text files; here the votes live in HBM
(tester.VoteAccumulator) and stay there.  Nothing of size N leaves the device: the one host read of a refinement is its
class counts together with the status words.

Everything is exact -- a 0/1 row is a bit set and a product of rows an AND, the comparison is a float32 widened to float64
against Python's double `0.01 * threshold`, counts are integers -- so the results equal the reference's, not approximately.

Anchors are CSR device tensors like active.anchor_scores' (anchor_ptr int64 [A + 1], anchor_idx int64 [nnz]); their label
rows `anchor_labels` are the host [A, C] 0/1 array of active.select_anchors.  C is the number of vote columns, one per
class that is not ignored: the label rows must have exactly the columns of the votes (ValueError otherwise); nothing is
padded or cut to fit.
"""
import warnings

import numpy as np
import torch

from . import _lib, ops
from ._lib import check, current_stream, ptr
from .active import MAX_CLASSES, _host_ids

STATUS_WORDS = 3
_STATUS_NAMES = ("anchor_idx holds %d point ids outside [0, n)",
                 "use_anchors holds %d anchor ids outside [0, A)",
                 "proj holds %d rows outside [0, M)")


def new_status(device):
    """the zeroed status words of the two kernels (weasal_hip.h: WS_REFINE_BAD_*), int64 [3] on the device"""
    return torch.zeros(STATUS_WORDS, dtype=torch.int64, device=device)


def pack_label_rows(anchor_labels):
    """host [A, C] 0/1 array -> uint32 [A], bit k = column k"""
    lb = np.asarray(anchor_labels)
    if lb.ndim != 2 or lb.shape[1] < 1:
        raise ValueError("anchor_labels must be [A, C]")
    if lb.shape[1] > MAX_CLASSES:
        raise ValueError("anchor_labels has %d columns (at most %d classes)" % (lb.shape[1], MAX_CLASSES))
    if not np.isin(lb, (0, 1)).all():
        raise ValueError("anchor_labels must hold zeros and ones")
    weights = np.uint64(1) << np.arange(lb.shape[1], dtype=np.uint64)
    return (lb.astype(np.uint64) * weights).sum(axis=1, dtype=np.uint64).astype(np.uint32)


def raise_on_status(words):
    """words: the host copy of the status words; ValueError naming the index lists that were out of range"""
    bad = [msg % int(v) for msg, v in zip(_STATUS_NAMES, words) if int(v) != 0]
    if bad:
        raise ValueError("pseudo-label refinement: " + "; ".join(bad) + " (skipped on the device)")


def read_counts(counts, status):
    """-> host int64 counts: the one host read of a refinement, counts and status words in a single copy"""
    n = counts.shape[0]
    host = torch.cat([counts.reshape(-1), status.reshape(-1)]).cpu().numpy()
    raise_on_status(host[n:])
    return host[:n].copy()


def weak_label_mask(n, anchor_ptr, anchor_idx, anchor_labels, use_anchors=None, status=None):
    """-> device uint32 [n], bit k set while class k survives at the point (pseudoLabel_refinement.py:63-68): all C bits
    for a point in no anchor, the AND of the label rows of the anchors that list it otherwise.  The number of classes
    travels with the tensor as `mask.classes`.

    use_anchors: host or device ids of the anchors that take part (the dictionary after active.select_anchors), any
    order, repeats allowed; None = all.  status: new_status() words shared with refine_labels; without them the call
    makes its own and reads them (a synchronising read), raising ValueError when an index was out of range."""
    lib = _lib.lib()
    ops._need_cuda(anchor_ptr, anchor_idx)
    bits = pack_label_rows(anchor_labels)
    c = np.asarray(anchor_labels).shape[1]
    ap = anchor_ptr.detach().to(torch.int64).contiguous()
    ai = anchor_idx.detach().to(torch.int64).contiguous()
    if ap.dim() != 1 or ap.shape[0] != bits.shape[0] + 1 or ai.dim() != 1:
        raise ValueError("anchor_ptr must have A + 1 entries for the A rows of anchor_labels, anchor_idx one dimension")
    dev = ap.device
    own = status is None
    if own:
        status = new_status(dev)
    ops._need_cuda(status)
    sel, n_sel = None, 0
    if use_anchors is not None:
        if isinstance(use_anchors, torch.Tensor) and use_anchors.is_cuda:
            sel = use_anchors.detach().reshape(-1).to(torch.int64).contiguous()
        else:
            sel = torch.from_numpy(_host_ids(use_anchors)).to(dev)
        n_sel = sel.shape[0]
        if n_sel == 0:                                       # an empty tensor has no pointer to tell "none" from "all"
            sel = torch.zeros(1, dtype=torch.int64, device=dev)
    mask = torch.empty(int(n), dtype=torch.uint32, device=dev)
    check(lib.ws_weak_mask(ptr(mask), int(n), c, ptr(ap), ptr(ai), ai.shape[0], ptr(torch.from_numpy(bits).to(dev)),
                           bits.shape[0], ptr(sel), n_sel, ptr(status), current_stream()))
    mask.classes = c
    if own:
        raise_on_status(status.cpu().numpy())
    return mask


def refine_labels(probs, preds, mask, threshold, proj=None, counts=None, no_label=10, out=None, status=None):
    """-> (labels int32 [N], counts int64 [n_counts]), both on the device (pseudoLabel_refinement.py:123-151).

    probs [M, C] float32 votes and preds [M] their label values; mask [N] from weak_label_mask; proj int32 [N]: the row of
    probs / preds that point i reads (None: row i).  labels[i] = no_label where the largest vote among the classes of
    mask[i] is below `threshold` percent (the double handed to the kernel is 0.01 * threshold), else preds[proj[i]].
    counts: labels counted by value into its n_counts bins, ADDED to what it holds, so that one buffer serves all tiles
    (None: a fresh zeroed buffer with one bin per class).  out: a contiguous int32 device tensor [N] written in place and
    returned -- the form SphereSampler keeps as its resident label buffer.  status: as in weak_label_mask."""
    lib = _lib.lib()
    if probs.dim() != 2:
        raise ValueError("probs must be [M, C]")
    classes = getattr(mask, "classes", None)
    if classes is not None and classes != probs.shape[1]:
        raise ValueError("the votes have %d columns, the weak-label mask was built for %d classes" % (probs.shape[1], classes))
    ops._need_cuda(probs, preds, mask, proj, counts, out, status)
    p = ops._f32c(probs)
    m, c = p.shape
    if mask.dtype != torch.uint32 or mask.dim() != 1 or not mask.is_contiguous():
        raise ValueError("mask must be a contiguous uint32 tensor [N] (weak_label_mask)")
    n = mask.shape[0]
    pr = preds.detach().reshape(-1).to(torch.int32).contiguous()
    if pr.shape[0] != m:
        raise ValueError("preds must hold one label per row of probs")
    pj = None
    if proj is not None:
        pj = proj.detach().reshape(-1).to(torch.int32).contiguous()
        if pj.shape[0] != n:
            raise ValueError("proj must hold one row index per point of the mask")
    elif m != n:
        raise ValueError("without proj the votes need one row per point: %d rows for %d points" % (m, n))
    if counts is None:
        counts = torch.zeros(c, dtype=torch.int64, device=p.device)
    elif counts.dtype != torch.int64 or counts.dim() != 1 or not counts.is_contiguous():
        raise ValueError("counts must be a contiguous int64 tensor (accumulated in place)")
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=p.device)
    elif out.dtype != torch.int32 or out.shape != (n,) or not out.is_contiguous():
        raise ValueError("out must be a contiguous int32 tensor [N] (written in place)")
    own = status is None
    if own:
        status = new_status(p.device)
    check(lib.ws_refine_labels(ptr(p), ptr(pr), m, c, ptr(mask), ptr(pj), n, 0.01 * threshold, int(no_label), ptr(out),
                               ptr(counts), counts.shape[0], ptr(status), current_stream()))
    if own:
        raise_on_status(status.cpu().numpy())
    return out, counts


def refine_cloud(votes, cloud, anchor_ptr, anchor_idx, anchor_labels, threshold, use_anchors=None, proj=None, counts=None,
                 no_label=10, out=None, label_values=None, ignored_labels=(), status=None):
    """One tile of pseudoLabel_refinement.py:54-151 from votes resident on the device: -> (labels int32 [N], counts), as
    refine_labels.  votes: a tester.VoteAccumulator; the votes are votes.probs[cloud], the predictions the label values
    of votes.predictions(cloud, label_values=..., ignored_labels=...).  N = the tile's point count, or len(proj).
    status: new_status() words to collect over several tiles and read once with read_counts(counts, status); without
    them the call reads its own (one synchronising read per call) and raises ValueError on an index out of range."""
    probs = votes.probs[cloud]
    lb = np.asarray(anchor_labels)
    if lb.ndim != 2 or lb.shape[1] != probs.shape[1]:
        raise ValueError("anchor_labels must be [A, C] with the C = %d columns of the votes" % probs.shape[1])
    ops._need_cuda(probs, anchor_ptr, anchor_idx, proj, counts, out, status)
    own = status is None
    if own:
        status = new_status(probs.device)
    n = probs.shape[0] if proj is None else proj.shape[0]
    mask = weak_label_mask(n, anchor_ptr, anchor_idx, lb, use_anchors, status)
    preds, _ = votes.predictions(cloud, label_values=label_values, ignored_labels=ignored_labels)
    labels, counts = refine_labels(probs, preds, mask, threshold, proj, counts, no_label, out, status)
    if own:
        raise_on_status(status.cpu().numpy())
    return labels, counts


def class_weights(counts):
    """pseudoLabel_refinement.py:168-169 on the host in float64: w = log(1 / ((counts + 1) / sum(counts))), w / sum(w).
    Warns, like the reference, when a class has no point."""
    if isinstance(counts, torch.Tensor):
        counts = counts.detach().cpu().numpy()
    counts = np.asarray(counts).astype(np.float64)
    if np.any(counts == 0):
        warnings.warn("pseudo labels: at least one class has count 0", RuntimeWarning, stacklevel=2)
    w = np.log(1.0 / ((counts + 1.0) / np.sum(counts)))
    return w / np.sum(w)


def write_pseudo_labels(path, labels):
    """one label per line, '%i': what np.genfromtxt(..., dtype=np.int32) of datasets/DALES_PseudoLabel.py:747 reads"""
    if isinstance(labels, torch.Tensor):
        labels = labels.detach().cpu().numpy()
    np.savetxt(path, np.asarray(labels).reshape(-1), fmt='%i')


def write_class_weights(path, weights):
    """one weight per line, '%.3f'"""
    np.savetxt(path, np.asarray(weights, dtype=np.float64).reshape(-1), fmt='%.3f')


def roundtrip_projection(full_points, sub_points, dl):
    """-> int32 [N_sub]: the index map of the reference's detour through the full-resolution prediction cloud
    (pseudoLabel_refinement.py:112-125): sub point -> its nearest full point -> that point's nearest sub point, each
    cloud reduced by its own minimum first (:112, :120).  dl: the cell of the grid subsampling that made sub_points (kept for the callers; the exact search does not read it).
    Optional: proj=None refines the sub-cloud votes directly, which is what tester.VoteAccumulator holds."""
    from . import tester
    ops._need_cuda(full_points, sub_points)
    full = ops._f32c(full_points)
    sub = ops._f32c(sub_points)
    full = full - full.amin(dim=0)
    sub = sub - sub.amin(dim=0)
    to_full = tester.nearest_projection(sub, full)           # the exact search: no radius to derive from dl
    back = tester.nearest_projection(full, sub)
    return back[to_full.long()].contiguous()
