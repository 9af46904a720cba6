"""Numpy restatement of the reference's per-epoch validation (utils/trainer_PseudoLabel.py:368-457, :503-541), in this
project's own words, with float64 votes like the reference's.  Host only: nothing here touches the device library.
The float32 softmax is torch's on the CPU, the one the reference takes."""
import numpy as np
import torch


def softmax32(logits):
    return torch.softmax(torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)), dim=1).numpy()


def vote_batch(votes, logits, lengths, inds, clouds, smooth=0.95, points=None, radius_mask=0.0):
    """votes: list of float64 [N_cloud, C], updated in place sphere after sphere (:391-407); with radius_mask > 0 only the
    rows with sum(points^2) < radius_mask^2 take part (the test loop's mask)"""
    probs = softmax32(logits)
    i0 = 0
    for n, cl in zip(lengths, clouds):
        rows = np.arange(i0, i0 + int(n))
        if radius_mask > 0:
            p = points[rows].astype(np.float32)
            rows = rows[((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]) < np.float32(radius_mask) ** 2]
        at = inds[rows]
        votes[cl][at] = smooth * votes[cl][at] + (1 - smooth) * probs[rows]
        i0 += int(n)
    return votes


def label_rows(label_values, ignored):
    """(row of a truth position, row of a vote column, kept rows) under fast_confusion's map: with label values that are
    not 0..n-1 the map sends a value to its rank and every absent value to 0 -- and the routine hands it truth POSITIONS"""
    lv = sorted(int(v) for v in label_values)
    n = len(lv)
    if lv == list(range(n)):
        rank = {v: v for v in range(n)}
    else:
        rank = {v: 0 for v in range(lv[-1] + 1)}
        rank.update({v: k for k, v in enumerate(lv)})
    kept = [k for k, v in enumerate(label_values) if int(v) not in set(int(i) for i in ignored)]
    return [rank[t] for t in range(n)], [rank[int(label_values[k])] for k in kept], kept


def batch_confusion(logits, labels, label_values, ignored):
    """int64 [n, n]: one count per row at (row of its truth position, row of its arg-max column)"""
    true_row, pred_row, _ = label_rows(label_values, ignored)
    best = np.argmax(softmax32(logits), axis=1)
    n = len(label_values)
    conf = np.zeros((n, n), np.int64)
    np.add.at(conf, (np.asarray(true_row)[labels], np.asarray(pred_row)[best]), 1)
    return conf


def balanced(conf, label_values, ignored, val_proportions):
    _, _, kept = label_rows(label_values, ignored)
    Cm = conf.astype(np.float32)[np.ix_(kept, kept)]
    Cm *= np.expand_dims(np.asarray(val_proportions, np.float32) / (np.sum(Cm, axis=1) + 1e-6), 1)
    return Cm


def iou(Cm):
    TP = np.diagonal(Cm)
    FN_TP, FP_TP = Cm.sum(axis=1), Cm.sum(axis=0)
    out = TP / (FP_TP + FN_TP - TP + 1e-6)
    absent = FN_TP < 1e-3
    return out + absent * (out.sum() / ((~absent).sum() + 1e-6))


def proportions(full_labels, label_values, ignored):
    return np.array([sum(int((lab == v).sum()) for lab in full_labels) for v in label_values if v not in ignored], np.float32)


def reprojected_confusion(votes, projs, full_labels, label_values, ignored):
    """(:503-537) arg-max of the votes (a point without votes takes the first label), re-projected, against label values"""
    label_values = np.asarray(label_values)
    _, _, kept = label_rows(label_values, ignored)
    n = len(label_values)
    rank = {int(v): k for k, v in enumerate(sorted(label_values))}
    conf = np.zeros((n, n), np.int64)
    for p, proj, lab in zip(votes, projs, full_labels):
        wide = np.zeros((p.shape[0], n))
        wide[:, kept] = p
        preds = label_values[np.argmax(wide, axis=1)][proj]
        np.add.at(conf, ([rank[int(v)] for v in lab], [rank[int(v)] for v in preds]), 1)
    return conf[np.ix_(kept, kept)]
