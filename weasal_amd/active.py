"""Active-learning selection on the device: from the votes of a pass over the training clouds to the ids of the next
ground-truth labels (csrc/active.hip).

Reference: utils/tester_PseudoLabel.py:393-438 (point labels: entropy * exp(class_w[arg-max]), descending, used ids removed,
the first `added_labels_per_epoch`) and utils/tester_WeakLabel.py:419-474 (weak region labels: mean entropy of an anchor
times the class scores of the classes predicted inside it).  The reference copies nothing because its votes already live
on the host; here they live in HBM (tester.VoteAccumulator) and stay there: scores, selection and the sort of the selected
ids are kernels, and the one host read of a selection is its k ids.

Order of a selection (ws_topk_select): descending score, ascending index among equal scores, -0.0 == +0.0, NaN last.

Opt-in, not in the reference (`min_spacing`, the configuration's `al_min_spacing`): the same order walked greedily with a
minimum distance between the new ids and to the used ones (spaced_top_k, ws_al_spaced_select).  Off, the default, nothing
here changes by an id or a launch.

The id lists (`used_ids`, `used_anchors`) are host int64 arrays, as in the reference, whose lists live in pickles between
iterations; device tensors are accepted and copied to the host.  Persisting them is the caller's business.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from ._lib import check, current_stream, ptr

MAX_CLASSES = 32


def _host_ids(ids):
    if ids is None:
        return np.zeros(0, np.int64)
    if isinstance(ids, torch.Tensor):
        ids = ids.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(ids).reshape(-1), dtype=np.int64)


def _class_score_dev(class_score, c, device):
    cs = np.ascontiguousarray(np.asarray(class_score, dtype=np.float64).reshape(-1))
    if cs.shape[0] != c:
        raise ValueError("class score has %d entries for %d classes" % (cs.shape[0], c))
    return torch.from_numpy(cs).to(device)


def point_scores(probs, class_w):
    """-> (entropy float32 [N], preds int32 [N], score float64 [N]) of votes `probs` [N, C] (a VoteAccumulator.probs[i]):
    tester_PseudoLabel.py:402-414.  class_w: the config's per-class weights (host); exp() of them is taken here, on the
    host in float64, so that it is the reference's exponential."""
    lib = _lib.lib()
    ops._need_cuda(probs)
    if probs.dim() != 2:
        raise ValueError("probs must be [N, C]")
    p = ops._f32c(probs)
    n, c = p.shape
    cs = _class_score_dev(np.exp(np.asarray(class_w, dtype=np.float64)), c, p.device)
    entropy = torch.empty(n, dtype=torch.float32, device=p.device)
    preds = torch.empty(n, dtype=torch.int32, device=p.device)
    score = torch.empty(n, dtype=torch.float64, device=p.device)
    check(lib.ws_al_point_scores(ptr(p), n, c, ptr(cs), ptr(entropy), ptr(preds), ptr(score), current_stream()))
    return entropy, preds, score


def anchor_scores(entropy, preds, anchor_ptr, anchor_idx, class_score):
    """-> float32 [A]: mean entropy of every anchor's points times the summed class score of the classes predicted inside
    it (tester_WeakLabel.py:436-454).  Anchors as CSR device tensors: anchor_ptr int64 [A + 1], anchor_idx int64 [nnz]."""
    lib = _lib.lib()
    ops._need_cuda(entropy, preds, anchor_ptr, anchor_idx)
    e = ops._f32c(entropy)
    pr = preds.detach().to(torch.int32).contiguous()
    ap = anchor_ptr.detach().to(torch.int64).contiguous()
    ai = anchor_idx.detach().to(torch.int64).contiguous()
    if e.shape[0] != pr.shape[0] or ap.dim() != 1 or ap.shape[0] < 1:
        raise ValueError("entropy / preds must have one entry per point, anchor_ptr A + 1 entries")
    na = ap.shape[0] - 1
    cs_host = np.asarray(class_score, dtype=np.float64).reshape(-1)
    cs = _class_score_dev(cs_host, cs_host.shape[0], e.device)
    out = torch.empty(na, dtype=torch.float32, device=e.device)
    check(lib.ws_al_anchor_scores(ptr(e), ptr(pr), e.shape[0], ptr(ap), ptr(ai), ai.shape[0], na, ptr(cs), cs.shape[0],
                                  ptr(out), current_stream()))
    return out


def top_k(score, k, exclude=None, exhausted=None):
    """-> device int64 [k]: the ids of the k largest scores that are not in `exclude`, in selection order (see the module
    docstring).  score: device float64 (float32 is widened, which is exact).  exclude: host or device ids, any order,
    duplicates allowed.  No result is read back here; the upload of the exclusion map waits for the work queued on the
    stream before it (weasal_hip.h).  The library walks the ids once: it rejects an id outside [0, n) (ValueError) and a k
    larger than what remains (ValueError(exhausted) when a message is given, else the library's error)."""
    lib = _lib.lib()
    ops._need_cuda(score)
    s = score.detach().reshape(-1).to(torch.float64).contiguous()
    ex = _host_ids(exclude)
    n, k = s.shape[0], int(k)
    ids = torch.empty(max(k, 0), dtype=torch.int64, device=s.device)
    scratch = torch.empty(lib.ws_topk_scratch_bytes(n, k), dtype=torch.uint8, device=s.device)
    rc = lib.ws_topk_select(ptr(s), n, C.c_void_p(ex.ctypes.data), ex.shape[0], k, ptr(ids), ptr(scratch), current_stream())
    if rc == 1:                                        # WS_ERR_INVALID, found on the host before anything was queued
        msg = (lib.ws_last_error() or b"").decode()
        if "not excluded" in msg and exhausted is not None:
            raise ValueError(exhausted)
        if "outside [0," in msg:
            raise ValueError("excluded ids: " + msg)
    check(rc)
    return ids


SPACED_PREFIX_FACTOR = 8      # default first run of spaced_top_k: max(SPACED_PREFIX_FACTOR * k, SPACED_PREFIX_MIN) candidates
SPACED_PREFIX_MIN = 4096
SPACED_PREFIX_GROWTH = 4      # every further run is this many times as long as the one before it
last_spaced = dict(passes=0, consumed=0)     # of the latest spaced_top_k call: runs taken, candidates handed to the walk


def _spacing(spacing):
    """None / 0 -> 0.0 (off); a finite value above 0 -> float; anything else: ValueError"""
    if spacing is None:
        return 0.0
    s = float(spacing)
    if not (np.isfinite(s) and s >= 0.0):
        raise ValueError("min_spacing must be None, 0 or a finite value above 0, got %r" % (spacing,))
    return s


def _coords_dev(coords, n, device):
    """float32 or float64 [n, 3], contiguous on `device` (host arrays, e.g. AnchorSet.centres, are uploaded)"""
    if coords is None:
        raise ValueError("a minimum spacing needs the coordinates of the scored items")
    c = coords if isinstance(coords, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(coords))
    if c.dtype not in (torch.float32, torch.float64):
        raise ValueError("coordinates must be float32 or float64, got %s" % c.dtype)
    if c.dim() != 2 or c.shape[0] != n or c.shape[1] != 3:
        raise ValueError("coordinates must be [%d, 3], got %s" % (n, tuple(c.shape)))
    return c.detach().to(device).contiguous()


def spaced_top_k(score, coords, k, spacing, exclude=None, exhausted=None, prefix=None):
    """-> device int64 [k]: top_k's priority order walked greedily with a minimum distance (ws_al_spaced_select): a
    candidate is accepted iff no id accepted before it and no id of `exclude` lies closer than `spacing` (float64
    d2 < spacing^2, strict); the accepted ids in acceptance order.  coords: [n, 3] float32 or float64, device tensor or
    host array.  spacing None or 0: top_k(score, k, exclude, exhausted) itself, nothing else is launched.

    The candidates come from top_k in runs: the first `prefix` not-excluded ids (default max(8 k, 4096), which makes one
    run the normal case: the walk ends within it unless more than 7 of 8 candidates are blocked), then, while fewer than k
    are accepted and candidates remain, a run four times as long that resumes the walk.  One blocking read per run: the
    acceptance count.  ValueError when every candidate is consumed with fewer than k accepted: `exhausted` (the
    reference's message) with the spacing appended.  `last_spaced` records the runs taken."""
    sp = _spacing(spacing)
    if sp == 0.0:
        return top_k(score, k, exclude, exhausted)
    lib = _lib.lib()
    ops._need_cuda(score)
    s = score.detach().reshape(-1).to(torch.float64).contiguous()
    n, k = s.shape[0], int(k)
    xyz = _coords_dev(coords, n, s.device)
    ex = _host_ids(exclude)
    if k < 0:
        raise ValueError("k = %d" % k)
    if ex.shape[0] and (ex.min() < 0 or ex.max() >= n):
        raise ValueError("excluded ids: outside [0, %d)" % n)
    free = n - np.unique(ex).shape[0]
    run = max(SPACED_PREFIX_FACTOR * k, SPACED_PREFIX_MIN) if prefix is None else int(prefix)
    if run < 1:
        raise ValueError("prefix = %d" % run)
    ids = torch.empty(k, dtype=torch.int64, device=s.device)
    state = torch.zeros(2, dtype=torch.int64, device=s.device)
    accepted = consumed = passes = 0
    while accepted < k and consumed < free:
        upto = min(free, consumed + run)
        cand = top_k(s, upto, ex)[consumed:]
        m = upto - consumed
        scratch = torch.empty(lib.ws_al_spaced_scratch_bytes(m, ex.shape[0], k), dtype=torch.uint8, device=s.device)
        check(lib.ws_al_spaced_select(ptr(xyz), int(xyz.dtype == torch.float64), n, ptr(cand), m, C.c_void_p(ex.ctypes.data),
                                      ex.shape[0], sp, k, ptr(ids), ptr(state), int(passes > 0), ptr(scratch), current_stream()))
        accepted = int(state[0].item())                # the one blocking read of a run
        consumed, passes, run = upto, passes + 1, run * SPACED_PREFIX_GROWTH
    last_spaced.update(passes=passes, consumed=consumed)
    if accepted < k:
        raise ValueError("%s (min_spacing %g: %d of %d found at that distance from each other and from the used ones)"
                         % (exhausted or "Not enough candidates left", sp, accepted, k))
    return ids


def select_points(votes, cloud, class_w, used_ids, k, points=None, min_spacing=0.0):
    """The next k point ids of `cloud` to receive their true label (tester_PseudoLabel.py:400-431): device int64 [k].
    votes: a tester.VoteAccumulator (or anything with .probs, a list of [N, C] device tensors).
    min_spacing above 0 (opt-in, not in the reference): no new id closer than that to another new one or to a used one
    (spaced_top_k); points: the cloud's [N, 3] coordinates (sampler.sub_points[cloud]), needed only then."""
    probs = votes.probs[cloud]
    ops._need_cuda(probs)
    spacing = _spacing(min_spacing)
    _, _, score = point_scores(probs, class_w)
    if spacing == 0.0:
        return top_k(score, k, used_ids, exhausted='Not enough point labels left for the next iteration')
    return spaced_top_k(score, points, k, spacing, used_ids, exhausted='Not enough point labels left for the next iteration')


def select_anchors(votes, cloud, anchor_ptr, anchor_idx, anchor_labels, used_anchors, k, centres=None, min_spacing=0.0):
    """The next k anchors of `cloud` to receive their weak label (tester_WeakLabel.py:410-467): device int64 [k].
    anchor_labels: host [A, C] 0/1 array (`anchor_lb`); used_anchors: the anchors used so far (`anchor_inds_sub`; every
    entry counts in label_sum, repeated or not, like the reference's loop).
    min_spacing above 0 (opt-in): no new anchor's centre closer than that to another new one's or a used one's
    (spaced_top_k); centres: [A, 3] (AnchorSet.centres), needed only then."""
    spacing = _spacing(min_spacing)
    probs = votes.probs[cloud]
    ops._need_cuda(probs, anchor_ptr, anchor_idx)
    used = _host_ids(used_anchors)
    lb = np.asarray(anchor_labels)
    na = int(anchor_ptr.shape[0]) - 1
    if lb.ndim != 2 or lb.shape[0] != na or lb.shape[1] != probs.shape[1]:
        raise ValueError("anchor_labels must be [A, C]")
    if used.shape[0] == 0:
        raise ValueError("select_anchors needs the anchors used so far: the class score divides by their number "
                         "(tester_WeakLabel.py:434)")
    if used.min() < 0 or used.max() >= na:
        raise ValueError("used anchors outside [0, %d)" % na)
    label_sum = lb[used].astype(np.int64).sum(axis=0)                     # :429-431
    class_score = np.exp(-label_sum / len(used))                          # :434
    entropy, preds, _ = point_scores(probs, np.zeros(probs.shape[1]))
    score = anchor_scores(entropy, preds, anchor_ptr, anchor_idx, class_score)
    if spacing == 0.0:
        return top_k(score, k, used, exhausted='Not enough weak labels left for the next iteration')
    return spaced_top_k(score, centres, k, spacing, used, exhausted='Not enough weak labels left for the next iteration')
