"""GPU: weasal_amd.anchors against the numpy restatement tests/anchors_ref.py -- equal, not close, in ptr, idx, bits, kept
and the order of the overlap anchors; the centres of the overlap anchors within n * 2^-52 * max|x| per coordinate (twice the
worst-case error of summing n float64 terms in any order, plus the division).  The cloud is anchors_ref.edge_cloud: 3002
points (no multiple of 64) with the cases listed there.  Every test imports weasal_amd.anchors, so all of them fail without
the feature."""
import numpy as np
import pytest
import torch

import anchors_ref
import refine_ref

pytestmark = pytest.mark.gpu
R = anchors_ref.RADIUS


@pytest.fixture(scope="module")
def cloud():
    points, labels, anchors = anchors_ref.edge_cloud()
    ref = anchors_ref.anchors_with_points(points, labels, anchors, R, 9)
    return points, labels, anchors, ref


@pytest.fixture(scope="module")
def built(cloud, gpu):
    from weasal_amd import anchors as wa
    points, labels, anchors, _ = cloud
    P, L = torch.from_numpy(points).to(gpu), torch.from_numpy(labels).to(gpu)
    return P, L, wa.anchors_with_points(P, L, anchors, R, 9)


def _host(aset):
    ptr, idx = aset.ptr.cpu().numpy(), aset.idx.cpu().numpy()
    return ptr, idx, aset.bits.cpu().numpy(), [idx[ptr[a]:ptr[a + 1]] for a in range(len(ptr) - 1)]


def _assert_set(aset, lists, lb, centres=None, n_base=None, points=None):
    ptr, idx, bits, got = _host(aset)
    want_ptr, want_idx = refine_ref.csr(lists)
    assert ptr.dtype == np.int64 and idx.dtype == np.int64 and bits.dtype == np.uint32
    assert np.array_equal(ptr, want_ptr) and np.array_equal(idx, want_idx)
    assert np.array_equal(bits, anchors_ref.pack_bits(lb)) and np.array_equal(aset.lb, lb)
    if centres is not None:
        assert aset.centres.dtype == np.float64 and aset.n_base == n_base
        assert np.array_equal(aset.centres[:n_base], centres[:n_base])
        p64 = np.asarray(points, np.float64)
        for a in range(n_base, len(lists)):
            m = p64[lists[a]]
            bound = len(m) * 2.0 ** -52 * np.abs(m).max(axis=0)
            assert np.all(np.abs(aset.centres[a] - centres[a]) <= bound), a


def test_the_cloud_holds_its_cases(cloud):
    points, labels, anchors, (kept, lists, centres, lb) = cloud
    sizes = np.array([len(l) for l in lists])
    assert points.shape[0] % 64 != 0 and 2900 < points.shape[0] < 3100
    assert sizes.max() > 1024 and ((sizes > 256) & (sizes <= 1024)).any() and (sizes == 1).any()
    missing = np.setdiff1d(np.arange(len(anchors)), kept)
    assert 0 in missing and len(anchors) - 1 in missing and len(missing) > 3
    on = int(np.nonzero((points == np.float32([3, 4, 0])).all(axis=1))[0][0])
    assert anchors_ref.d2_to(points[on:on + 1], anchors[1])[0] == 25.0 and on in lists[int(np.nonzero(kept == 1)[0][0])]
    out = int(np.nonzero((points == np.float32([400, 5, 0])).all(axis=1))[0][0])
    d2 = anchors_ref.d2_to(points[out:out + 1], anchors[7])[0]
    assert 25.0 < d2 < 25.0 + 1e-13 and float(points[out, 1]) - anchors[7, 1] == np.nextafter(5.0, 6.0)
    assert out not in lists[int(np.nonzero(kept == 7)[0][0])]


def test_bounds_and_lattice(cloud, gpu):
    from weasal_amd import anchors as wa
    points = cloud[0]
    P = torch.from_numpy(points).to(gpu)
    want = np.array([f(points[:, d]) for d in range(3) for f in (np.min, np.max)], np.float32)
    assert np.array_equal(wa.cloud_bounds(P), want)
    slab = points[(points[:, 0] >= 700) & (points[:, 0] <= 750)]
    S = torch.from_numpy(slab).to(gpu)
    for method in ("full", "reduced"):
        got = wa.get_anchors(S, R, method)
        assert got.dtype == np.float64 and np.array_equal(got, anchors_ref.get_anchors(slab, R, method))
    with pytest.raises(ValueError, match="Unsupported method"):
        wa.get_anchors(S, R, "half")
    one = torch.tensor([[-0.5, 2.0, 1e30]], device=gpu)
    assert np.array_equal(wa.cloud_bounds(one), np.float32([-0.5, -0.5, 2.0, 2.0, 1e30, 1e30]))


def test_members_equal_the_restatement(cloud, built):
    _, _, anchors, (kept, lists, centres, lb) = cloud
    aset = built[2]
    assert np.array_equal(aset.kept, kept) and aset.kept.dtype == np.int64 and np.array_equal(aset.centres, centres)
    _assert_set(aset, lists, lb)
    assert len(aset) == len(kept) and aset.n_base == len(kept) and aset.n_class == 9


def test_thirty_two_classes(cloud, gpu):
    from weasal_amd import anchors as wa
    points, labels, anchors, _ = cloud
    lab = labels.copy()
    lab[::7] = 31
    lab[1::11] = 17
    kept, lists, centres, lb = anchors_ref.anchors_with_points(points, lab, anchors, R, 32)
    assert lb[:, 31].any()
    aset = wa.anchors_with_points(torch.from_numpy(points).to(gpu), torch.from_numpy(lab).to(gpu), anchors, R, 32)
    assert np.array_equal(aset.kept, kept)
    _assert_set(aset, lists, lb)
    with pytest.raises(ValueError, match="n_class"):
        wa.anchors_with_points(torch.from_numpy(points).to(gpu), torch.from_numpy(lab).to(gpu), anchors, R, 33)


def test_a_label_out_of_range_raises(cloud, gpu):
    from weasal_amd import anchors as wa
    points, labels, anchors, _ = cloud
    lab = labels.copy()
    lab[5], lab[77] = 9, -1
    with pytest.raises(ValueError, match="labels holds 2 values outside"):
        wa.anchors_with_points(torch.from_numpy(points).to(gpu), torch.from_numpy(lab).to(gpu), anchors, R, 9)


def test_one_anchor_and_none(cloud, built):
    from weasal_amd import anchors as wa
    P, L, _ = built
    for anchors in (np.zeros((0, 3)), np.array([[1000.0, 1000.0, 1000.0]])):
        aset = wa.anchors_with_points(P, L, anchors, R, 9)
        assert len(aset) == 0 and aset.ptr.cpu().tolist() == [0] and aset.idx.shape[0] == 0 and aset.lb.shape == (0, 9)
        assert aset.kept.shape == (0,) and aset.centres.shape == (0, 3)
        again = wa.update_anchors(aset, P, R)
        assert len(again) == 0 and again.ptr.cpu().tolist() == [0]
    hit = wa.anchors_with_points(P, L, np.array([[0.0, 0.0, 0.0]]), R, 9)
    assert len(hit) == 1 and hit.kept.tolist() == [0] and hit.ptr.cpu().tolist() == [0, 2] and hit.lb[0].tolist() == [0, 0, 1] + [0] * 6
    assert len(wa.update_anchors(hit, P, R)) == 1


def test_overlap_anchors_equal_the_restatement(cloud, built):
    from weasal_amd import anchors as wa
    points, _, _, (kept, lists, centres, lb) = cloud
    P, _, aset = built
    ol, oc, olb, n_base = anchors_ref.update_anchors(points, lists, centres, lb, R)
    new = [len(l) for l in ol[n_base:]]
    assert 1 in new and max(new) > 256 and len(new) > 10
    pos = {int(a): k for k, a in enumerate(kept)}
    pairs = anchors_ref.candidate_pairs(centres, R)
    for i, j, same_rows, common in ((8, 9, True, 2), (10, 11, False, 0), (12, 13, False, 1), (2, 3, False, 1100)):
        assert (pos[i], pos[j]) in pairs and np.array_equal(lb[pos[i]], lb[pos[j]]) == same_rows
        assert len(np.intersect1d(lists[pos[i]], lists[pos[j]])) == common
    got = wa.update_anchors(aset, P, R)
    _assert_set(got, ol, olb, oc, n_base, points)
    assert np.array_equal(got.kept, kept)


def test_overlap_anchors_of_a_selection(cloud, built):
    from weasal_amd import anchors as wa
    points, _, _, (kept, lists, centres, lb) = cloud
    P, _, aset = built
    rng = np.random.RandomState(3)
    sel = np.sort(rng.choice(len(lists), size=60, replace=False))
    sel = np.concatenate([[sel[10]], sel, [sel[10], 2, 3]])                     # duplicates, out of order
    ol, oc, olb, n_base = anchors_ref.update_anchors(points, lists, centres, lb, R, use_anchors=sel)
    assert len(ol) > n_base
    for use in (sel, torch.from_numpy(sel).to(P.device), sel.tolist()):
        got = wa.update_anchors(aset, P, R, use_anchors=use)
        _assert_set(got, ol, olb, oc, n_base, points)
        assert np.array_equal(got.kept, kept[sel])
    picked = wa.select_anchors(aset, sel)
    _assert_set(picked, ol[:n_base], olb[:n_base])


def test_a_selection_out_of_range_raises_and_writes_nothing(cloud, built):
    from weasal_amd import anchors as wa
    P, _, aset = built
    before = [t.clone() for t in (aset.ptr, aset.idx, aset.bits)]
    for bad in ([0, len(aset)], [-1, 2]):
        with pytest.raises(ValueError, match="use_anchors holds 1 anchor ids outside"):
            wa.update_anchors(aset, P, R, use_anchors=bad)
        with pytest.raises(ValueError, match="use_anchors holds 1 anchor ids outside"):
            wa.select_anchors(aset, bad)
    torch.cuda.synchronize()
    for a, b in zip(before, (aset.ptr, aset.idx, aset.bits)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_two_builds_give_the_same_bytes(cloud, built):
    from weasal_amd import anchors as wa
    anchors = cloud[2]
    P, L, first = built
    second = wa.anchors_with_points(P, L, anchors, R, 9)
    a, b = wa.update_anchors(first, P, R), wa.update_anchors(second, P, R)
    for x, y in ((first, second), (a, b)):
        for name in ("ptr", "idx", "bits"):
            assert getattr(x, name).cpu().numpy().tobytes() == getattr(y, name).cpu().numpy().tobytes(), name
        assert x.centres.tobytes() == y.centres.tobytes() and x.lb.tobytes() == y.lb.tobytes() and x.kept.tobytes() == y.kept.tobytes()


def test_save_and_load(built, tmp_path):
    from weasal_amd import anchors as wa
    P, _, aset = built
    full = wa.update_anchors(aset, P, R)
    path = str(tmp_path / "tile_anchors.npz")
    full.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ["bits", "centres", "idx", "kept", "lb", "n_base", "ptr"]
    back = wa.AnchorSet.load(path, P.device)
    assert back.n_base == full.n_base and torch.equal(back.ptr, full.ptr) and torch.equal(back.idx, full.idx)
    assert np.array_equal(back.bits.cpu().numpy(), full.bits.cpu().numpy())
    assert np.array_equal(back.centres, full.centres) and np.array_equal(back.lb, full.lb) and np.array_equal(back.kept, full.kept)


def test_the_set_feeds_the_weak_label_mask(cloud, built):
    from weasal_amd import anchors as wa, refine
    points, _, _, (kept, lists, centres, lb) = cloud
    P, _, aset = built
    full = wa.update_anchors(aset, P, R)
    ol, _, olb, _ = anchors_ref.update_anchors(points, lists, centres, lb, R)
    ptr, idx = refine_ref.csr(ol)
    n = points.shape[0]
    for use in (None, [0, 5, 5, len(ol) - 1]):
        want = refine_ref.mask_bits(refine_ref.weak_labels(n, ptr, idx, olb, use))
        got = refine.weak_label_mask(n, full.ptr, full.idx, full.lb, use_anchors=use)
        assert np.array_equal(got.cpu().numpy(), want)
