"""CPU (no GPU needed): the restatement tests/regions_ref.py of the weak-label sampler's sub-regions against golden
g17_regions.npz (the reference's own body of datasets/DALES_WeakLabel.py:418-451 on anchors built by its utils/anchors.py), the
row-0 rule (`if idx.any()`, :449) on hand-made lists, the layout of regions.SphereRegions.to_lists, and the C ABI of
csrc/regions.hip: the entries resolve and refuse bad sizes before the device is touched."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import anchors_ref
import regions_ref
from conftest import golden


def _digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def golden_anchor_set(g):
    ptr, idx = g["a_ptr"], g["a_idx"]
    return [idx[ptr[a]:ptr[a + 1]] for a in range(len(ptr) - 1)], g["a_lb"], g["a_centres"]


def golden_record(g, k):
    """the recorded regions of sphere k as a sorted list of (tile point ids, label row)"""
    ptr, ids, lb = g["s%d_ptr" % k], g["s%d_ids" % k], g["s%d_lb" % k]
    return sorted((tuple(ids[ptr[r]:ptr[r + 1]]), tuple(int(v) for v in lb[r])) for r in range(len(ptr) - 1))


def test_restatement_reproduces_the_reference_record():
    g = golden("g17_regions.npz")
    points, labels = anchors_ref.golden_cloud()
    assert np.array_equal(_digest(points), g["points_sha"]) and np.array_equal(_digest(labels), g["labels_sha"])
    aset = golden_anchor_set(g)
    assert len(aset[0]) == 112 and int(g["n_base"]) == 64
    r = regions_ref.search_radius(float(g["in_radius"]), float(g["sub_radius"]))
    assert r == 14.0 - 5.0 - 0.01
    counts = []
    for k, centre in enumerate(g["centres"]):
        inds = regions_ref.sphere_inds(points, centre, float(g["in_radius"]))
        assert len(inds) == int(g["s%d_n" % k])
        ids, regs, rows = regions_ref.sphere_regions(aset, centre, inds, r)
        assert ids == sorted(ids)
        mine = sorted((tuple(inds[x]), tuple(int(v) for v in row)) for x, row in zip(regs, rows))
        assert mine == golden_record(g, k)
        counts.append((len(inds), len(regs)))
    assert counts[0] == (956, 17) and counts[-1] == (0, 0)


def test_row_zero_rule():
    inds = np.array([3, 8, 9, 20, 21, 40], np.int64)
    assert regions_ref.region_of([3], inds) is None                                  # {row 0}: dropped
    assert regions_ref.region_of([3, 40], inds).tolist() == [0, 5]                   # {row 0, row 5}: kept with both
    assert regions_ref.region_of([5, 7, 100], inds) is None                          # nothing inside: dropped
    assert regions_ref.region_of([], inds) is None
    assert regions_ref.region_of([8], inds).tolist() == [1]                          # a single member that is not row 0
    assert regions_ref.region_of([2, 8, 21, 22], inds).tolist() == [1, 4]            # partly outside
    aset = ([np.array([3]), np.array([3, 40]), np.array([5, 7]), np.array([9, 20])], np.eye(4, dtype=np.int64), np.zeros((4, 3)))
    c = regions_ref.cut([aset], [0], np.zeros((1, 3)), inds, [6], np.zeros(6, np.int64), 10.0, 4.0, 4)
    assert c["anchor"].tolist() == [1, 3] and c["ptr"].tolist() == [0, 2, 4] and c["idx"].tolist() == [0, 5, 2, 3]
    assert np.array_equal(c["lb"], np.eye(4, dtype=np.float32)[[1, 3]]) and c["cloud_lb"].tolist() == [[1, 0, 0, 0]]
    t_ptr, t_reg = regions_ref.transpose(c["ptr"], c["idx"], 6)
    assert t_ptr.tolist() == [0, 1, 1, 2, 3, 3, 4] and t_reg.tolist() == [0, 1, 1, 0]


def test_to_lists_layout():
    """three spheres of 4, 3 and 5 rows; regions: sphere 0 {1, 3}, sphere 2 {0, 4} and {2}; sphere 1 has none"""
    from weasal_amd.regions import SphereRegions
    ptr = np.array([0, 2, 4, 5], np.int64)
    idx = np.array([1, 3, 7, 11, 9], np.int64)                                       # rows of the stacked batch
    lb = np.array([[1, 0], [0, 1], [1, 1]], np.float32)
    sr = SphereRegions(ptr, idx, np.array([0, 0, 1, 1, 2], np.int32), np.array([0, 2, 2], np.int32), np.array([5, 1, 6], np.int64), lb,
                       np.array([0.5, 0.5, 1.0], np.float32), None, None, None, [4, 3, 5], 3, 5)
    assert len(sr) == 3 and sr.n_regions == 3 and sr.n_rows == 12
    region, region_lb = sr.to_lists()
    assert [len(r) for r in region] == [1, 0, 2] and [len(r) for r in region_lb] == [1, 0, 2]
    assert region[0][0].tolist() == [1, 3] and region[2][0].tolist() == [0, 4] and region[2][1].tolist() == [2]
    assert all(a.dtype == np.int64 for r in region for a in r)
    assert all(a.dtype == np.float32 and a.shape == (2,) for r in region_lb for a in r)
    assert region_lb[0][0].tolist() == [1, 0] and region_lb[2][0].tolist() == [0, 1] and region_lb[2][1].tolist() == [1, 1]


def test_abi_entries_resolve_and_validate_without_a_device():
    from weasal_amd import _lib
    lib = _lib.lib()
    names = ("ws_region_scratch_bytes", "ws_region_cut_count", "ws_region_cut_scan", "ws_region_cut_fill", "ws_region_mean_fwd",
             "ws_region_mean_bwd")
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    null, one = C.c_void_p(None), C.c_void_p(16)                                     # never dereferenced: validation fails first
    assert lib.ws_region_scratch_bytes(0) >= 4 and lib.ws_region_scratch_bytes(100000) > 4 * 100000
    assert lib.ws_region_mean_fwd(one, 8, 257, one, one, 4, one, 2, one, null) == 2 and b"257" in lib.ws_last_error()
    assert lib.ws_region_mean_bwd(one, 2, 0, one, one, 4, one, 8, one, null) == 2
    assert lib.ws_region_mean_fwd(one, 8, 36, one, one, 4, one, 0, one, null) == 0    # no region: nothing is queued
    assert lib.ws_region_mean_fwd(one, -1, 36, one, one, 4, one, 2, one, null) == 1
    assert lib.ws_region_cut_scan(one, 10, one, one, one, one, 8, 65, 9, one, one, one, null) == 2     # more than 64 spheres
    assert lib.ws_region_cut_scan(one, 10, one, one, one, one, 8, 2, 33, one, one, one, null) == 2     # more than 32 classes
    assert lib.ws_region_cut_count(one, one, one, 4, 0, one, 1, 1, one, one, one, one, 8, 0, 5.0, one, null) == 1   # no anchors
    assert lib.ws_region_cut_fill(one, one, 4, one, 3, one, 1, 1, one, one, one, 8, 3, one, one, one, 0, 0, 9, one, one, one, one, one,
                                  one, one, null) == 0                                                 # no region: nothing is queued
    with pytest.raises(ValueError, match="256"):
        from weasal_amd import ops
        ops._region_width(257)
