"""CPU restatement (numpy) of the pseudo-label refinement, the yardstick of tests/test_refine_*.py and the host side of
tools/refine_bench.py.  Written from the arithmetic of pseudoLabel_refinement.py:63-68 (per-point weak labels), :123-145
(projection, emptying), :148-151 (counts by value) and :168-169 (class weights); nothing here touches the device library.

Anchors are CSR (anchor_ptr [A + 1], anchor_idx [nnz]) with the 0/1 label rows anchor_labels [A, C], in place of the
reference's dictionary of index lists.  Every step is exact, so the tests compare for equality.
"""
import numpy as np


def weak_labels(n, anchor_ptr, anchor_idx, anchor_labels, use_anchors=None):
    """float64 [n, C] of zeros and ones: ones, then weak[idx_a] *= lb_a for every anchor that takes part (:63-68).  The
    fancy-indexed product applies a row once to an index that its list repeats; an anchor repeated in use_anchors
    multiplies by the same zeros and ones again, which changes nothing."""
    lb = np.asarray(anchor_labels)
    weak = np.ones((n, lb.shape[1]))
    rows = range(len(anchor_ptr) - 1) if use_anchors is None else use_anchors
    for a in rows:
        idx = np.asarray(anchor_idx[anchor_ptr[a]:anchor_ptr[a + 1]], np.int64)
        weak[idx] = weak[idx] * lb[a]
    return weak


def mask_bits(weak):
    """uint32 [n]: bit k set where weak[:, k] is one (the device's form of the same table; C <= 32)"""
    w = np.asarray(weak)
    return (w.astype(np.uint64) << np.arange(w.shape[1], dtype=np.uint64)).sum(axis=1, dtype=np.uint64).astype(np.uint32)


def refine(probs, preds, weak, threshold, proj=None, n_counts=None, no_label=10):
    """(labels int32 [N], counts int64 [n_counts]) of one tile: probs [M, C] float32 votes, preds [M] their label values,
    weak [N, C] the table of weak_labels(), proj [N] the row of probs / preds a point reads (None: its own).  The weak
    labels belong to the point itself and are not projected (:136-137)."""
    p = np.asarray(probs, np.float32)
    labels = np.asarray(preds).astype(np.int32)
    if proj is not None:
        p, labels = p[proj], labels[proj]                                    # :136, :144
    else:
        labels = labels.copy()
    empty = np.max(p * weak, axis=-1) < (0.01 * threshold)                   # :137, :143
    labels[empty] = no_label                                                 # :145
    n_counts = p.shape[1] if n_counts is None else n_counts
    counts = np.zeros(n_counts, np.int64)
    values, counter = np.unique(labels, return_counts=True)                  # :148-151: by value, after emptying
    for c in range(n_counts):
        if c in values:
            counts[c] += counter[np.where(values == c)][0]
    return labels, counts


def class_weights(counts):
    """:168-169"""
    counts = np.asarray(counts, np.int64)
    with np.errstate(divide='ignore'):
        w = np.log(1 / ((counts + 1) / np.sum(counts)))
    return w / np.sum(w)


def refine_cloud(probs, label_values, n, anchor_ptr, anchor_idx, anchor_labels, threshold, use_anchors=None, proj=None,
                 n_counts=None, no_label=10):
    """one tile from its votes alone: the predictions are the label values at the arg-max of the votes"""
    p = np.asarray(probs, np.float32)
    preds = np.asarray(label_values)[np.argmax(p, axis=1)]
    weak = weak_labels(n, anchor_ptr, anchor_idx, anchor_labels, use_anchors)
    return refine(p, preds, weak, threshold, proj, n_counts, no_label)


# ------------------------------------------------------------------------------------------------------------------
# fixtures shared by the GPU tests and tools/refine_bench.py
# ------------------------------------------------------------------------------------------------------------------
def csr(lists):
    """(anchor_ptr int64 [A + 1], anchor_idx int64 [nnz]) of a list of index lists"""
    ptr = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(l) for l in lists], out=ptr[1:])
    idx = np.concatenate([np.asarray(l, np.int64).reshape(-1) for l in lists] + [np.zeros(0, np.int64)])
    return ptr, idx


def nearest_brute(queries, support, chunk=512):
    """(index int64 [Q], exact ties bool [Q]) of the nearest support point of every query, float32 squared distances
    (dx*dx + dy*dy) + dz*dz; `ties` marks the queries whose two smallest distances are equal"""
    q = np.asarray(queries, np.float32)
    s = np.asarray(support, np.float32)
    out = np.empty(len(q), np.int64)
    ties = np.zeros(len(q), bool)
    for a in range(0, len(q), chunk):
        d = q[a:a + chunk, None, :] - s[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        out[a:a + chunk] = np.argmin(d2, axis=1)
        if s.shape[0] > 1:
            two = np.partition(d2, 1, axis=1)[:, :2]
            ties[a:a + chunk] = two[:, 0] == two[:, 1]
    return out, ties
