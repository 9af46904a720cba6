"""numpy restatement of the reference's test run (utils/tester_PseudoLabel.py:87-449, utils/tester_WeakLabel.py:87-485) for
tests/golden/g21_test_run.npz and for the kernel tests: the checkpoint rule, np.insert, arg-max, fast_confusion, the error
map and the fields of the written files.  Not collected; nothing here is used by the product."""
import hashlib
import os

import numpy as np


# ------------------------------------------------------------------------------------------------------------------
# the loop (:141-149, :214-223, :268, :446)
# ------------------------------------------------------------------------------------------------------------------
def run_rule(minima, num_votes):
    """-> [(test_epoch, checkpoint, reproject)] for a sequence of per-epoch minimum potentials, until the loop breaks;
    the last entry has no successor.  ended: whether the loop broke inside the sequence."""
    last_min = -0.5
    steps = []
    for e, new_min in enumerate(minima):
        checkpoint = reproject = False
        if last_min + 1 < new_min:
            last_min += 1
            checkpoint = True
            if last_min > num_votes:
                reproject = True
        steps.append((e, checkpoint, reproject))
        if last_min > num_votes:
            return steps, True
    return steps, False


# ------------------------------------------------------------------------------------------------------------------
# votes (:168-195)
# ------------------------------------------------------------------------------------------------------------------
def vote_update(test_probs, softmaxed, points, lengths, in_inds, cloud_inds, in_radius, test_radius_ratio=0.7, test_smooth=0.95):
    i0 = 0
    for b_i, length in enumerate(lengths):
        pts = points[i0:i0 + length]
        probs = softmaxed[i0:i0 + length]
        inds = in_inds[i0:i0 + length]
        c_i = cloud_inds[b_i]
        if 0 < test_radius_ratio < 1:
            mask = np.sum(pts ** 2, axis=1) < (test_radius_ratio * in_radius) ** 2
            inds = inds[mask]
            probs = probs[mask]
        test_probs[c_i][inds] = test_smooth * test_probs[c_i][inds] + (1 - test_smooth) * probs
        i0 += length
    return test_probs


# ------------------------------------------------------------------------------------------------------------------
# the outputs (:231-244, :277, :297-307, :343-348)
# ------------------------------------------------------------------------------------------------------------------
def expand(probs, label_values, ignored_labels):
    for l_ind, label_value in enumerate(label_values):
        if label_value in ignored_labels:
            probs = np.insert(probs, l_ind, 0, axis=1)
    return probs


def fast_confusion(true, pred, label_values):
    """utils/metrics.py:35-110 for 1-D int arrays and given label values"""
    true = np.asarray(true).astype(np.int32)
    pred = np.asarray(pred).astype(np.int32)
    label_values = np.sort(np.asarray(label_values))
    num_classes = len(label_values)
    if not (label_values[0] == 0 and label_values[-1] == num_classes - 1):
        label_map = np.zeros((label_values[-1] + 1,), dtype=np.int32)
        for k, v in enumerate(label_values):
            label_map[v] = k
        pred = label_map[pred]
        true = label_map[true]
    vec_conf = np.bincount(true * num_classes + pred)
    if vec_conf.shape[0] < num_classes ** 2:
        vec_conf = np.pad(vec_conf, (0, num_classes ** 2 - vec_conf.shape[0]), 'constant')
    return vec_conf.reshape((num_classes, num_classes))


def IoU_from_confusions(confusions):
    """utils/metrics.py:204-230"""
    TP = np.diagonal(confusions, axis1=-2, axis2=-1)
    TP_plus_FN = np.sum(confusions, axis=-1)
    TP_plus_FP = np.sum(confusions, axis=-2)
    IoU = TP / (TP_plus_FP + TP_plus_FN - TP + 1e-6)
    mask = TP_plus_FN < 1e-3
    counts = np.sum(1 - mask, axis=-1, keepdims=True)
    mIoU = np.sum(IoU, axis=-1, keepdims=True) / (counts + 1e-6)
    IoU += mask * mIoU
    return IoU


def cloud_outputs(votes, proj, label_values, ignored_labels, targets=None):
    """one cloud, the reference's lines: -> (proj_probs [m, c_all] in the dtype of the votes, preds int32, error int8 or
    None, fast_confusion or None).  proj None: the sub-cloud itself."""
    label_values = np.asarray(label_values)
    probs = np.array(votes, copy=True) if proj is None else votes[proj, :]
    probs = expand(probs, label_values, ignored_labels)
    preds = label_values[np.argmax(probs, axis=1)].astype(np.int32)
    if targets is None:
        return probs, preds, None, None
    error_map = (preds != targets).astype('int8')
    return probs, preds, error_map, fast_confusion(targets, preds, label_values)


def strip(C, label_values, ignored_labels):
    for l_ind, label_value in reversed(list(enumerate(label_values))):
        if label_value in ignored_labels:
            C = np.delete(C, l_ind, axis=0)
            C = np.delete(C, l_ind, axis=1)
    return C


def score_line(IoUs):
    s = '{:5.2f} | '.format(100 * np.mean(IoUs))
    for IoU in IoUs:
        s += '{:5.2f} '.format(100 * IoU)
    return s


def sub_checkpoint(votes, sub_labels, label_values, ignored_labels, val_proportions):
    """"Confusion on sub clouds" (:225-264) -> (summed raw confusion, balanced float32 matrix, IoUs, printed line)"""
    Confs = [cloud_outputs(v, None, label_values, ignored_labels, t)[3] for v, t in zip(votes, sub_labels)]
    raw = np.sum(np.stack(Confs), axis=0)
    C = strip(raw.astype(np.float32), label_values, ignored_labels)
    C *= np.expand_dims(val_proportions / (np.sum(C, axis=1) + 1e-6), 1)
    IoUs = IoU_from_confusions(C)
    return raw, C, IoUs, score_line(IoUs)


def full_clouds(votes, projs, full_labels, label_values, ignored_labels):
    """(:270-328) -> (per cloud (proj_probs, preds, error, conf), summed raw confusion, stripped matrix, IoUs, line)"""
    outs = [cloud_outputs(v, p, label_values, ignored_labels, t) for v, p, t in zip(votes, projs, full_labels)]
    raw = np.sum(np.stack([o[3] for o in outs]), axis=0)
    C = strip(raw, label_values, ignored_labels)
    IoUs = IoU_from_confusions(C)
    return outs, raw, C, IoUs, score_line(IoUs)


def write_files(directory, write_ply, cloud_names, full_points, coord_offset, outs, full_labels, label_names):
    """the files of :350-361 through the given writer"""
    for sub in ('predictions', 'probs'):
        os.makedirs(os.path.join(directory, sub), exist_ok=True)
    prob_names = ['_'.join(n.split()) for n in label_names]
    for name, pts, (probs, preds, error, _), targets in zip(cloud_names, full_points, outs, full_labels):
        points = pts + coord_offset
        write_ply(os.path.join(directory, 'predictions', name), [points, preds, targets, error], ['x', 'y', 'z', 'preds', 'targets', 'error'])
        write_ply(os.path.join(directory, 'probs', name), [points, probs], ['x', 'y', 'z'] + prob_names)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------------------------
# ws_test_outputs as the header states it, status words included
# ------------------------------------------------------------------------------------------------------------------
def kernel_outputs(votes, proj, col_of, label_values, targets=None, true_row=None, confusion=None):
    """-> (proj_probs [m, c_all], preds int32 [m], error int8 [m] or None, confusion int64 [c_all, c_all] or None,
    status int64 [2]).  confusion: the matrix to accumulate into (a copy is returned)."""
    votes = np.asarray(votes)
    n_sub, c = votes.shape
    label_values = np.asarray(label_values)
    c_all = len(label_values)
    idx = np.arange(n_sub, dtype=np.int64) if proj is None else np.asarray(proj).astype(np.int64)
    m = len(idx)
    ok = (idx >= 0) & (idx < n_sub)
    rows = votes[np.where(ok, idx, 0)]
    rows[~ok] = 0
    probs = np.zeros((m, c_all), votes.dtype)
    probs[:, np.asarray(col_of)] = rows
    best = np.argmax(probs, axis=1)
    preds = label_values[best].astype(np.int32)
    status = np.array([int((~ok).sum()), 0], np.int64)
    if targets is None:
        return probs, preds, None, None, status
    targets = np.asarray(targets)
    error = (preds != targets).astype(np.int8)
    if true_row is None:
        return probs, preds, error, None, status
    true_row = np.asarray(true_row)
    inside = (targets >= 0) & (targets < len(true_row))
    tr = np.where(inside, true_row[np.where(inside, targets, 0)], -1)
    good = (tr >= 0) & (tr < c_all)
    status[1] = int((~good).sum())
    use = good & ok
    conf = np.zeros((c_all, c_all), np.int64) if confusion is None else np.array(confusion, dtype=np.int64, copy=True)
    np.add.at(conf, (tr[use], best[use]), 1)
    return probs, preds, error, conf, status
