"""CPU (no GPU needed): the numpy restatement of the pseudo-label refinement (tests/refine_ref.py) on a case small enough
to write out by hand, the host half of weasal_amd.refine (class weights, the text files, the packing of label rows), and
the argument validation of the two library entries, which happens before the device is touched."""
import ctypes as C
import warnings

import numpy as np
import pytest

import refine_ref

# 6 points, 3 classes, 3 anchors.  Every vote is a binary fraction and the threshold is 25 %: 0.01 * 25 == 0.25 exactly.
PTR, IDX = refine_ref.csr([[0, 1, 1],            # a duplicate index inside a list
                           [1, 2, 4],            # point 1 is in two anchors with disjoint labels
                           []])                  # an empty anchor
LABELS = np.array([[1, 0, 0], [0, 1, 1], [0, 0, 0]], np.int64)                # points 3 and 5 are in no anchor
PROBS = np.array([[0.125, 0.75, 0.125],
                  [1.0, 0.0, 0.0],
                  [0.5, 0.25, 0.25],
                  [0.0, 0.0, 0.0],
                  [0.25, 0.5, 0.25],
                  [0.125, 0.125, 0.75]], np.float32)
PREDS = np.array([1, 0, 0, 0, 1, 2], np.int32)                                # np.argmax of the rows


def test_restatement_on_a_hand_sized_case():
    assert 0.01 * 25 == 0.25
    assert PTR.tolist() == [0, 3, 6, 6] and IDX.tolist() == [0, 1, 1, 1, 2, 4]
    weak = refine_ref.weak_labels(6, PTR, IDX, LABELS)
    assert weak.tolist() == [[1, 0, 0], [0, 0, 0], [0, 1, 1], [1, 1, 1], [0, 1, 1], [1, 1, 1]]
    assert refine_ref.mask_bits(weak).tolist() == [1, 0, 6, 7, 6, 7]
    # point 0: its arg-max class is not allowed, the allowed one has 0.125 < 0.25: emptied.  point 1: nothing allowed.
    # point 2: predicted 0, which its weak labels exclude -- the label is NOT masked, only the test is -- and the largest
    # allowed vote is 0.25, not below 0.25: kept.  point 3: never voted on.
    labels, counts = refine_ref.refine(PROBS, PREDS, weak, 25)
    assert labels.dtype == np.int32 and counts.dtype == np.int64
    assert labels.tolist() == [10, 10, 0, 10, 1, 2] and counts.tolist() == [1, 1, 1]
    assert refine_ref.refine(PROBS, PREDS, weak, 25, n_counts=11)[1].tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 3]
    assert refine_ref.refine(PROBS, PREDS, weak, 25, n_counts=2, no_label=1)[0].tolist() == [1, 1, 0, 1, 1, 2]
    assert refine_ref.refine(PROBS, PREDS, weak, 25, n_counts=2, no_label=1)[1].tolist() == [1, 4]
    assert refine_ref.refine(PROBS, PREDS, weak, 0)[0].tolist() == PREDS.tolist()          # nothing is below 0
    # a projection moves votes and predictions, not the weak labels
    proj = np.array([5, 5, 2, 3, 0, 1])
    labels, counts = refine_ref.refine(PROBS, PREDS, weak, 25, proj=proj)
    assert labels.tolist() == [10, 10, 0, 10, 1, 0] and counts.tolist() == [2, 1, 0]
    # only anchor 1, named twice
    weak1 = refine_ref.weak_labels(6, PTR, IDX, LABELS, use_anchors=[1, 1])
    assert weak1.tolist() == [[1, 1, 1], [0, 1, 1], [0, 1, 1], [1, 1, 1], [0, 1, 1], [1, 1, 1]]
    assert refine_ref.refine(PROBS, PREDS, weak1, 25)[0].tolist() == [1, 10, 0, 10, 1, 2]
    assert refine_ref.weak_labels(6, PTR, IDX, LABELS, use_anchors=[]).min() == 1
    # the same tile from its votes alone, with label values 1..3
    labels, counts = refine_ref.refine_cloud(PROBS, [1, 2, 3], 6, PTR, IDX, LABELS, 25, n_counts=4)
    assert labels.tolist() == [10, 10, 1, 10, 2, 3] and counts.tolist() == [0, 1, 1, 1]


def test_pack_label_rows_is_the_restatements_bit_table():
    from weasal_amd import refine
    rng = np.random.default_rng(0)
    for c in (1, 9, 32):
        lb = (rng.random((50, c)) < 0.5).astype(np.int64)
        lb[0], lb[1] = 0, 1
        bits = refine.pack_label_rows(lb)
        assert bits.dtype == np.uint32 and np.array_equal(bits, refine_ref.mask_bits(lb))
        assert bits[0] == 0 and int(bits[1]) == (1 << c) - 1
    assert refine.pack_label_rows(LABELS).tolist() == [1, 6, 0]
    with pytest.raises(ValueError):
        refine.pack_label_rows(np.ones((2, 33)))
    with pytest.raises(ValueError):
        refine.pack_label_rows(np.full((2, 3), 2))
    with pytest.raises(ValueError):
        refine.pack_label_rows(np.ones(3))


def test_class_weights_and_the_text_files(tmp_path):
    from weasal_amd import refine
    counts = np.array([5, 0, 15, 1234567], np.int64)
    total = 5 + 0 + 15 + 1234567
    w = np.log(np.array([total / 6, total / 1, total / 16, total / 1234568]))
    want = w / w.sum()
    with pytest.warns(RuntimeWarning, match="count 0"):
        got = refine.class_weights(counts)
    assert got.dtype == np.float64
    assert np.allclose(got, want, rtol=1e-14, atol=0) and abs(got.sum() - 1) < 1e-15
    assert np.array_equal(got, refine_ref.class_weights(counts))                  # the expression itself, operation by operation
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        refine.class_weights(np.array([3, 1, 2]))                                 # no empty class: no warning
    labels = np.array([0, 10, 8, 3, 10, 10, 1], np.int32)
    lp, wp = tmp_path / "tile_t10_pseudo.txt", tmp_path / "DALES_t10_weight.txt"
    refine.write_pseudo_labels(str(lp), labels)
    refine.write_class_weights(str(wp), got)
    assert open(lp).read().split() == ["0", "10", "8", "3", "10", "10", "1"]
    back = np.genfromtxt(str(lp), dtype=np.int32)
    assert back.dtype == np.int32 and np.array_equal(back, labels)
    text = open(wp).read().split()
    assert text == ["%.3f" % v for v in got] and all(len(t.split(".")[1]) == 3 for t in text)
    assert np.array_equal(np.genfromtxt(str(wp)), np.round(got, 3))


def test_refine_entries_validate_before_touching_the_device():
    from weasal_amd import _lib
    lib = _lib.lib()
    null = C.c_void_p(None)
    one = C.c_void_p(16)     # never dereferenced: validation fails first
    # ws_weak_mask(mask, n, c, anchor_ptr, anchor_idx, nnz, anchor_bits, n_anchors, anchor_sel, n_sel, status, stream)
    assert lib.ws_weak_mask(one, 4, 33, one, one, 8, one, 2, null, 0, one, null) == 2 and b"at most 32" in lib.ws_last_error()
    assert lib.ws_weak_mask(one, 4, 0, one, one, 8, one, 2, null, 0, one, null) == 1
    assert lib.ws_weak_mask(null, 0, 3, null, null, 0, null, 0, null, 0, null, null) == 0
    assert lib.ws_weak_mask(null, 4, 3, one, one, 8, one, 2, null, 0, one, null) == 1 and b"NULL" in lib.ws_last_error()
    assert lib.ws_weak_mask(one, 4, 3, one, one, 8, one, 2, null, 0, null, null) == 1
    assert lib.ws_weak_mask(one, 4, 3, null, one, 8, one, 2, null, 0, one, null) == 1
    assert lib.ws_weak_mask(one, 4, 3, one, null, 8, one, 2, null, 0, one, null) == 1
    assert lib.ws_weak_mask(one, 4, 3, one, one, 8, null, 2, null, 0, one, null) == 1
    assert lib.ws_weak_mask(one, 4, 3, one, one, 8, one, 2, null, 5, one, null) == 1          # a count without a list
    for bad in ((-1, 8, 2, 0), (4, -1, 2, 0), (4, 8, -2, 0), (4, 8, 2, -1)):
        n, nnz, na, ns = bad
        assert lib.ws_weak_mask(one, n, 3, one, one, nnz, one, na, one, ns, one, null) == 1
    # ws_refine_labels(probs, preds, m, c, mask, proj, n, thr, no_label, labels, counts, n_counts, status, stream)
    assert lib.ws_refine_labels(one, one, 4, 33, one, null, 4, 0.1, 10, one, one, 9, one, null) == 2
    assert b"at most 32" in lib.ws_last_error()
    assert lib.ws_refine_labels(one, one, 4, 0, one, null, 4, 0.1, 10, one, one, 9, one, null) == 1
    assert lib.ws_refine_labels(null, null, 0, 9, null, null, 0, 0.1, 10, null, null, 9, null, null) == 0
    assert lib.ws_refine_labels(one, one, 4, 9, one, null, 4, 0.1, 10, one, one, 5000, one, null) == 2
    assert lib.ws_refine_labels(one, one, 4, 9, one, null, -1, 0.1, 10, one, one, 9, one, null) == 1
    assert lib.ws_refine_labels(one, one, -4, 9, one, one, 4, 0.1, 10, one, one, 9, one, null) == 1
    assert lib.ws_refine_labels(one, one, 4, 9, one, null, 4, 0.1, 10, one, one, -1, one, null) == 1
    for k in (0, 1, 4, 9, 10, 12):                                                           # each required pointer
        args = [one, one, 4, 9, one, null, 4, 0.1, 10, one, one, 9, one, null]
        args[k] = null
        assert lib.ws_refine_labels(*args) == 1 and b"NULL" in lib.ws_last_error(), k
    # without a projection every point needs its own row of votes
    assert lib.ws_refine_labels(one, one, 3, 9, one, null, 4, 0.1, 10, one, one, 9, one, null) == 1
    assert b"row per point" in lib.ws_last_error()


class Votes:
    def __init__(self, probs):
        self.probs = [probs]


def test_python_entry_points_refuse_cpu_tensors():
    import torch
    from weasal_amd import _lib, refine
    ptr, idx = torch.from_numpy(PTR), torch.from_numpy(IDX)
    with pytest.raises(_lib.WeasalHipError):
        refine.weak_label_mask(6, ptr, idx, LABELS)
    with pytest.raises(_lib.WeasalHipError):
        refine.refine_labels(torch.from_numpy(PROBS), torch.from_numpy(PREDS), torch.zeros(6, dtype=torch.uint32), 25)
    with pytest.raises(_lib.WeasalHipError):
        refine.refine_cloud(Votes(torch.from_numpy(PROBS)), 0, ptr, idx, LABELS, 25)
    with pytest.raises(_lib.WeasalHipError):
        refine.roundtrip_projection(torch.zeros(8, 3), torch.zeros(4, 3), 0.5)


def test_vote_columns_must_be_the_columns_of_the_label_rows():
    import torch
    from weasal_amd import refine
    ptr, idx = torch.from_numpy(PTR), torch.from_numpy(IDX)
    for c in (2, 4):
        with pytest.raises(ValueError, match="columns of the votes"):
            refine.refine_cloud(Votes(torch.zeros(6, c)), 0, ptr, idx, LABELS, 25)
    mask = torch.zeros(6, dtype=torch.uint32)
    mask.classes = 3
    with pytest.raises(ValueError, match="built for 3 classes"):
        refine.refine_labels(torch.zeros(6, 4), torch.zeros(6, dtype=torch.int32), mask, 25)
