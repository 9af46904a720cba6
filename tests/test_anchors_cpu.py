"""CPU (no GPU needed): the numpy restatement tests/anchors_ref.py against the golden g16_anchors.npz recorded from the
reference's utils/anchors.py, and the host-only parts of weasal_amd.anchors (lattice from bounds, subsampling, label bits)."""
import hashlib
import random

import numpy as np
import pytest

import anchors_ref
from conftest import golden


@pytest.fixture(scope="module")
def g16():
    g = golden("g16_anchors.npz")
    points, labels = anchors_ref.golden_cloud()
    for a, name in ((points, "points_sha"), (labels, "labels_sha")):
        assert hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest() == g[name].tobytes()
    return g, points, labels


@pytest.fixture(scope="module")
def base(g16):
    g, points, labels = g16
    return anchors_ref.anchors_with_points(points, labels, g["anchors_reduced"], float(g["sub_radius"]), int(g["n_class"]))


def _lists(ptr, idx):
    return [idx[ptr[a]:ptr[a + 1]] for a in range(len(ptr) - 1)]


def _same_multiset(points, got_lists, got_lb, got_centres, want_lists, want_lb, want_centres):
    """overlap anchors as a multiset of (index list, label row), centres within n * 2^-52 * max|x| per coordinate: twice
    the worst-case error of summing n float64 terms in any order, plus the division"""
    def key(l, r):
        return tuple(int(v) for v in l), tuple(int(v) for v in r)
    got = sorted(range(len(got_lists)), key=lambda k: key(got_lists[k], got_lb[k]))
    want = sorted(range(len(want_lists)), key=lambda k: key(want_lists[k], want_lb[k]))
    assert [key(got_lists[k], got_lb[k]) for k in got] == [key(want_lists[k], want_lb[k]) for k in want]
    p64 = np.asarray(points, np.float64)
    for a, b in zip(got, want):
        m = p64[np.asarray(got_lists[a], np.int64)]
        bound = len(m) * 2.0 ** -52 * np.abs(m).max(axis=0)
        assert np.all(np.abs(got_centres[a] - want_centres[b]) <= bound)


def test_lattice_equals_the_reference(g16):
    from weasal_amd import anchors
    g, points, _ = g16
    bounds = np.array([f(points[:, d]) for d in range(3) for f in (np.min, np.max)], np.float32)
    for method in ("full", "reduced"):
        want = g["anchors_" + method]
        assert np.array_equal(anchors_ref.get_anchors(points, 5.0, method), want)
        got = anchors.anchors_from_bounds(bounds, 5.0, method)
        assert got.dtype == np.float64 and np.array_equal(got, want)
    with pytest.raises(ValueError, match="Unsupported method"):
        anchors.anchors_from_bounds(bounds, 5.0, "half")
    with pytest.raises(ValueError, match="Unsupported method"):
        anchors_ref.get_anchors(points, 5.0, "half")


def test_base_anchors_equal_the_reference(g16, base):
    g, _, _ = g16
    kept, lists, centres, lb = base
    assert np.array_equal(kept, g["kept"]) and np.array_equal(lb, g["lb"]) and np.array_equal(centres, g["centres"])
    ptr = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(l) for l in lists], out=ptr[1:])
    assert np.array_equal(ptr, g["member_ptr"]) and np.array_equal(np.concatenate(lists), g["member_idx"])


def test_overlap_anchors_equal_the_reference_as_a_multiset(g16, base):
    g, points, _ = g16
    _, lists, centres, lb = base
    ol, oc, olb, n_base = anchors_ref.update_anchors(points, lists, centres, lb, 5.0)
    assert n_base == len(lists) and len(ol) - n_base == len(g["ov_ptr"]) - 1 > 20
    _same_multiset(points, ol[n_base:], olb[n_base:], oc[n_base:], _lists(g["ov_ptr"], g["ov_idx"]), g["ov_lb"], g["ov_centres"])
    pairs = anchors_ref.candidate_pairs(centres, 5.0)
    assert pairs == sorted(pairs) and all(i < j for i, j in pairs)


def test_overlap_anchors_of_a_subset_with_a_duplicate(g16, base):
    g, points, _ = g16
    _, lists, centres, lb = base
    sel = g["sel"]
    assert len(set(sel.tolist())) < len(sel)
    ol, oc, olb, n_base = anchors_ref.update_anchors(points, lists, centres, lb, 5.0, use_anchors=sel)
    assert n_base == len(sel) and all(np.array_equal(ol[k], lists[a]) for k, a in enumerate(sel))
    _same_multiset(points, ol[n_base:], olb[n_base:], oc[n_base:], _lists(g["sel_ov_ptr"], g["sel_ov_idx"]), g["sel_ov_lb"],
                   g["sel_ov_centres"])
    with pytest.raises(ValueError):
        anchors_ref.update_anchors(points, lists, centres, lb, 5.0, use_anchors=[0, len(lists)])


@pytest.mark.parametrize("method", ["regular", "random", "balanced"])
def test_subsample_indices_equal_the_reference(g16, base, method):
    from weasal_amd import anchors
    g, _, _ = g16
    lb = base[3]
    for fn in (anchors_ref.subsample_indices, anchors.subsample_indices):
        random.seed(int(g["seed_sub"]))
        got = np.asarray(fn(lb, int(g["sub_count"]), method), np.int64)
        assert np.array_equal(got, g["sub_" + method]), fn.__module__
    if method != "regular":
        random.seed(int(g["seed_sub"]) + 1)
        assert not np.array_equal(np.asarray(anchors.subsample_indices(lb, int(g["sub_count"]), method)), g["sub_" + method])


def test_subsample_value_errors(base):
    from weasal_amd import anchors
    lb = base[3]
    for fn in (anchors_ref.subsample_indices, anchors.subsample_indices):
        with pytest.raises(ValueError, match="exceeds the number of anchors"):
            fn(lb, len(lb) + 1, "regular")
        with pytest.raises(ValueError, match="is not supported"):
            fn(lb, 5, "stratified")


def test_label_bits_round_trip(base):
    from weasal_amd import anchors, refine
    lb = base[3]
    bits = anchors_ref.pack_bits(lb)
    assert np.array_equal(bits, refine.pack_label_rows(lb))
    rows = anchors.unpack_label_bits(bits, lb.shape[1])
    assert np.array_equal(rows, lb) and np.array_equal(refine.pack_label_rows(rows), bits)
    wide = np.zeros((3, 32), np.int64)
    wide[0, 31] = wide[1, 0] = wide[2, 17] = 1
    assert np.array_equal(anchors.unpack_label_bits(refine.pack_label_rows(wide), 32), wide)


def test_linspace_is_numpys():
    from weasal_amd import anchors
    for lo, hi, num in ((np.float32(0.1), np.float32(41.7), 9), (-3.25, 3.25, 2), (1.5, 1.5, 4), (2.0, 7.0, 1), (0.0, 1e-320, 3)):
        assert np.array_equal(anchors._linspace(lo, hi, num), np.linspace(np.float64(lo), np.float64(hi), num))
