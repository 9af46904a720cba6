"""CPU restatement (numpy) of the active-learning selection, the yardstick of tests/test_active_*.py and the host side of
tools/active_bench.py.  Written from the arithmetic of utils/tester_PseudoLabel.py:400-431 and
utils/tester_WeakLabel.py:410-467; nothing here touches the device library.

Two forms of the removal of used ids are given: `remove_used_reference`, the reference's loop (one np.delete(np.where())
per used id, O(used * N)), and a mask (`select`), which yields the same list; the tests check that they agree and then use
the mask.  The order of equal scores is pinned to ascending index (np.lexsort), the project's tie rule: the reference's
np.argsort(-score) is a quicksort, whose order of equal scores is unspecified.
"""
import numpy as np


def entropy(probs):
    """float32 [N]: -sum_k p_k * log2(p_k + 1e-12) on the float32 votes (numpy keeps float32 throughout)"""
    p = np.asarray(probs, np.float32)
    return -np.sum(p * np.log2(p + np.float32(1e-12)), axis=1)


def point_scores(probs, class_w):
    """(entropy f32 [N], preds [N], score f64 [N]): entropy * exp(class_w[arg-max])"""
    p = np.asarray(probs, np.float32)
    h = entropy(p)
    preds = np.argmax(p, axis=1)
    class_scores = np.exp(np.asarray(class_w, dtype=np.float64)[preds])
    return h, preds, h * class_scores


def order(score):
    """all ids: descending score, ascending index among equal scores, -0.0 == +0.0, NaN last"""
    s = np.asarray(score, np.float64)
    idx = np.arange(s.shape[0])
    nan = np.isnan(s)
    key = np.where(nan, 0.0, -s) + 0.0                    # (-0.0 + 0.0 = +0.0)
    return np.lexsort((idx, key, nan)).astype(np.int64)


def remove_used_reference(sort_ids, used):
    """the reference's loop over the used ids"""
    for u in used:
        sort_ids = np.delete(sort_ids, np.where(sort_ids == u))
    return sort_ids


def select(score, used, k, message='Not enough point labels left for the next iteration'):
    """the first k ids of order(score) that are not in `used`"""
    ids = order(score)
    keep = np.ones(ids.shape[0], bool)
    keep[np.asarray(used, np.int64)] = False
    ids = ids[keep[ids]]
    if len(ids) < k:
        raise ValueError(message)
    return ids[:k]


def select_points(probs, class_w, used, k):
    return select(point_scores(probs, class_w)[2], used, k)


def anchor_class_score(anchor_labels, used):
    """exp(-label_sum / len(used)): label_sum counts the classes of every used anchor"""
    lb = np.asarray(anchor_labels)
    label_sum = np.zeros(lb.shape[1], dtype=np.int64)
    for a in used:
        label_sum += lb[a]
    return np.exp(-label_sum / len(used))


def anchor_scores(probs, anchor_ptr, anchor_idx, class_scores):
    """float32 [A]: mean entropy of the anchor's points times the summed class score of the classes predicted in it"""
    p = np.asarray(probs, np.float32)
    h = entropy(p)
    preds = np.argmax(p, axis=1)
    out = np.zeros(len(anchor_ptr) - 1, np.float32)
    for a in range(len(out)):
        ids = anchor_idx[anchor_ptr[a]:anchor_ptr[a + 1]]
        if len(ids) == 0:
            continue
        present = np.zeros(p.shape[1], dtype=np.int64)
        present[np.unique(preds[ids])] = 1
        out[a] = np.mean(h[ids]) * np.matmul(present, class_scores)
    return out


def select_anchors(probs, anchor_ptr, anchor_idx, anchor_labels, used, k):
    cs = anchor_class_score(anchor_labels, used)
    score = anchor_scores(probs, anchor_ptr, anchor_idx, cs)
    return select(score, used, k, 'Not enough weak labels left for the next iteration')


# ------------------------------------------------------------------------------------------------------------------
# fixtures shared by the GPU tests and tools/active_bench.py
# ------------------------------------------------------------------------------------------------------------------
def synthetic_votes(seed, n, c=9, unvoted=0.03, sharp=3.0):
    """float32 [n, c] votes the way a voting pass leaves them: softmax rows scaled by 1 - smooth^v for v = 1..6 visits,
    and a fraction `unvoted` of rows that no sphere reached (all zeros)"""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((n, c)) * sharp).astype(np.float32)
    e = np.exp(logits - logits.max(1, keepdims=True))
    p = (e / e.sum(1, keepdims=True)).astype(np.float32)
    visits = rng.integers(1, 7, size=n)
    p *= (1.0 - 0.95 ** visits).astype(np.float32)[:, None]
    p[rng.random(n) < unvoted] = 0.0
    return p


def synthetic_anchors(seed, n, n_anchors, c=9, lo=50, hi=4000):
    """(anchor_ptr int64 [A + 1], anchor_idx int64, anchor_labels int64 [A, c]): anchors of lo..hi points, each a run of
    consecutive ids from a random start (a region of a spatially ordered cloud), shuffled inside"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi + 1, size=n_anchors)
    ptr = np.zeros(n_anchors + 1, np.int64)
    np.cumsum(sizes, out=ptr[1:])
    idx = np.empty(ptr[-1], np.int64)
    for a, m in enumerate(sizes):
        start = rng.integers(0, n - m + 1)
        idx[ptr[a]:ptr[a + 1]] = start + rng.permutation(m)
    labels = (rng.random((n_anchors, c)) < 0.3).astype(np.int64)
    return ptr, idx, labels
