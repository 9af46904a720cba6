"""CPU (no GPU needed): the numpy restatement of the active-learning selection (tests/active_ref.py) on a case small
enough to write out by hand, and the argument validation of the library's selection entries, which happens before the
device is touched."""
import ctypes as C

import numpy as np
import pytest

import active_ref


def test_restatement_on_a_hand_sized_case():
    # every probability is a power of two: log2 is exact and 1e-12 vanishes in float32 next to it
    probs = np.array([[0.5, 0.25, 0.25],        # H = 1.5, class 0
                      [1.0, 0.0, 0.0],          # H = 0,   class 0
                      [0.25, 0.25, 0.5],        # H = 1.5, class 2
                      [0.25, 0.5, 0.25]],       # H = 1.5, class 1
                     np.float32)
    class_w = [0.0, 1.0, 0.0]
    h, preds, score = active_ref.point_scores(probs, class_w)
    assert h.dtype == np.float32 and score.dtype == np.float64
    assert h.tolist() == [1.5, 0.0, 1.5, 1.5]
    assert preds.tolist() == [0, 0, 2, 1]
    assert score[[0, 1, 2]].tolist() == [1.5, 0.0, 1.5] and score[3] == pytest.approx(4.077422742688568, rel=1e-15)
    assert active_ref.order(score).tolist() == [3, 0, 2, 1]                  # the tie 0 / 2 in index order
    assert active_ref.select(score, [], 4).tolist() == [3, 0, 2, 1]
    assert active_ref.select(score, [0], 2).tolist() == [3, 2]
    assert active_ref.select(score, [2, 0, 2], 2).tolist() == [3, 1]         # duplicates in the used list
    with pytest.raises(ValueError, match='Not enough point labels left for the next iteration'):
        active_ref.select(score, [0, 3], 3)
    # first maximum on a tie, and a row nobody voted on
    h2, p2, s2 = active_ref.point_scores(np.array([[0.5, 0.5, 0.0], [0, 0, 0]], np.float32), class_w)
    assert h2.tolist() == [1.0, 0.0] and p2.tolist() == [0, 0] and s2.tolist() == [1.0, 0.0]


def test_restatement_order_rules_and_the_reference_removal_loop():
    s = np.array([0.5, np.nan, -0.0, 0.0, 0.5, -np.inf, np.inf, np.nan, -1.0])
    assert active_ref.order(s).tolist() == [6, 0, 4, 2, 3, 8, 5, 1, 7]
    rng = np.random.default_rng(0)
    score = np.round(rng.standard_normal(500) * 64) / 64
    used = rng.integers(0, 500, size=60)
    want = active_ref.remove_used_reference(active_ref.order(score), used)[:100]
    assert np.array_equal(active_ref.select(score, used, 100), want)


def test_restatement_anchors_on_a_hand_sized_case():
    probs = np.array([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0], [0.25, 0.25, 0.5], [0.25, 0.5, 0.25]], np.float32)
    ptr = np.array([0, 2, 2, 5], np.int64)
    idx = np.array([0, 1, 3, 2, 0], np.int64)
    labels = np.array([[1, 0, 0], [0, 1, 0], [1, 0, 1]], np.int64)
    cs = active_ref.anchor_class_score(labels, [0, 0])                        # label_sum = [2, 0, 0] over two entries
    assert cs.tolist() == [np.exp(-1.0), 1.0, 1.0]
    out = active_ref.anchor_scores(probs, ptr, idx, np.array([0.5, 2.0, 4.0]))
    assert out.dtype == np.float32
    assert out.tolist() == [0.75 * 0.5, 0.0, 1.5 * 6.5]                       # classes {0}, none, {0, 1, 2}
    with pytest.raises(ValueError, match='Not enough weak labels left for the next iteration'):
        active_ref.select_anchors(probs, ptr, idx, labels, [0, 1], 2)


def _host(a):
    return C.c_void_p(a.ctypes.data)


def test_selection_entries_validate_before_touching_the_device():
    from weasal_amd import _lib
    lib = _lib.lib()
    null = C.c_void_p(None)
    one = C.c_void_p(16)     # never dereferenced: validation fails first
    # point scores
    assert lib.ws_al_point_scores(null, 4, 3, one, one, one, one, null) == 1 and b"NULL" in lib.ws_last_error()
    assert lib.ws_al_point_scores(one, 4, 3, one, one, null, one, null) == 1
    assert lib.ws_al_point_scores(one, 4, 33, one, one, one, one, null) == 2 and b"at most 32" in lib.ws_last_error()
    assert lib.ws_al_point_scores(one, -1, 3, one, one, one, one, null) == 1
    assert lib.ws_al_point_scores(null, 0, 3, null, null, null, null, null) == 0
    # anchor scores
    assert lib.ws_al_anchor_scores(one, one, 4, null, one, 8, 2, one, 3, one, null) == 1 and b"NULL" in lib.ws_last_error()
    assert lib.ws_al_anchor_scores(one, one, 4, one, one, 8, 2, one, 3, null, null) == 1
    assert lib.ws_al_anchor_scores(one, one, 4, one, one, 8, 2, one, 33, one, null) == 2
    assert lib.ws_al_anchor_scores(null, null, 4, null, null, 0, 0, null, 3, null, null) == 0
    # top-k: the excluded ids are a host array, checked on the host
    dup = np.array([1, 1, 2], np.int64)
    assert lib.ws_topk_select(one, 10, _host(dup), 3, 9, one, one, null) == 1 and b"not excluded" in lib.ws_last_error()
    assert lib.ws_topk_select(null, 10, _host(dup), 3, 8, one, one, null) == 1 and b"NULL" in lib.ws_last_error()
    assert lib.ws_topk_select(one, 10, _host(dup), 3, 8, null, one, null) == 1
    assert lib.ws_topk_select(one, 10, _host(dup), 3, 8, one, null, null) == 1
    assert lib.ws_topk_select(one, 10, null, 0, 11, one, one, null) == 1
    assert lib.ws_topk_select(one, 10, null, 3, 1, one, one, null) == 1
    for bad in (10, -1, 1 << 40):
        ex = np.array([3, bad], np.int64)
        assert lib.ws_topk_select(one, 10, _host(ex), 2, 1, one, one, null) == 1 and b"outside" in lib.ws_last_error()
    assert lib.ws_topk_select(one, 10, null, 0, -1, one, one, null) == 1
    assert lib.ws_topk_select(null, 0, null, 0, 0, null, null, null) == 0
    assert lib.ws_topk_select(null, 0, null, 0, 1, null, null, null) == 1
    assert lib.ws_topk_select(null, 10, _host(dup), 3, 0, null, null, null) == 0          # nothing asked for


def test_topk_scratch_grows_with_n_and_k():
    from weasal_amd import _lib
    lib = _lib.lib()
    ns = [0, 1, 1000, 4097, 300000, (1 << 21) + 3, 1 << 24]
    ks = [0, 1, 200, 2049, 5000, 65536, 1 << 21]
    table = np.array([[lib.ws_topk_scratch_bytes(n, k) for k in ks] for n in ns])
    assert (table > 0).all()
    assert (np.diff(table, axis=0) >= 0).all() and (np.diff(table, axis=1) >= 0).all()
    assert table[-1, -1] > table[0, 0]
    # room for the keys of every candidate and for a (key, id) pair of every survivor, twice (the sort's two buffers)
    assert lib.ws_topk_scratch_bytes(300000, 5000) >= 300000 * 8 + 2 * 5000 * 12


def test_python_entry_points_refuse_cpu_tensors():
    import torch
    from weasal_amd import _lib, active

    class Votes:
        probs = [torch.zeros(8, 3)]
    with pytest.raises(_lib.WeasalHipError):
        active.point_scores(torch.zeros(8, 3), [0, 0, 0])
    with pytest.raises(_lib.WeasalHipError):
        active.top_k(torch.zeros(8, dtype=torch.float64), 2)
    with pytest.raises(_lib.WeasalHipError):
        active.anchor_scores(torch.zeros(8), torch.zeros(8, dtype=torch.int32), torch.zeros(2, dtype=torch.int64),
                             torch.zeros(4, dtype=torch.int64), [1, 1, 1])
    with pytest.raises(_lib.WeasalHipError):
        active.select_points(Votes(), 0, [0, 0, 0], [], 2)
    with pytest.raises(_lib.WeasalHipError):
        active.select_anchors(Votes(), 0, torch.zeros(2, dtype=torch.int64), torch.zeros(4, dtype=torch.int64),
                              np.zeros((1, 3)), [0], 1)
