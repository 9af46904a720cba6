"""Per-epoch validation on the device (weasal_amd/validation.py, csrc/validation.hip): one launch per batch, one blocking
read per epoch.  Held to tests/golden/g19_validation.npz (the reference's own routine), to the per-sphere path of
tester.VoteAccumulator.update, and to the numpy restatement tests/validation_ref.py.

The bound on votes, 2e-6 absolute, is the one tests/test_tester.py holds this float32 arithmetic to over a chain of the
same length (a float32 chain of six updates against float64 differs by about 6e-8; swapping two updates at smooth = 0.95
moves a vote by (1 - smooth)^2 * |a2 - a1|, 2.5e-5 at the least on the golden's rows)."""
import numpy as np
import pytest
import torch

import validation_ref as ref
from conftest import golden

pytestmark = pytest.mark.gpu
BOUND = 2e-6


def _dev(gpu):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


# ---------------------------------------------------------------------------------------------------------------
# 1. the reference's routine
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["A", "B"])
def test_golden_replay(gpu, tag, tmp_path):
    from weasal_amd import validation
    g, dev = golden("g19_validation.npz"), _dev(gpu)
    lv, ign, sizes = g[tag + "/label_values"], g[tag + "/ignored"], g[tag + "/cloud_sizes"]
    full = [g["%s/full_labels_%d" % (tag, i)] for i in range(len(sizes))]
    v = validation.Validator(sizes, lv, ign, [dev(a) for a in full], gpu)
    assert v.val_proportions.dtype == np.float32 and np.array_equal(v.val_proportions, g[tag + "/val_proportions"])
    for epoch in range(2):
        for k in range(3):
            key = "%s/e%d/b%d/" % (tag, epoch, k)
            v.update(dev(g[key + "logits"]), {"labels": dev(g[key + "labels"]), "lengths": g[key + "lengths"],
                                              "input_inds": dev(g[key + "inds"]), "cloud_inds": g[key + "clouds"]})
        syncs = v._sync_count
        ious, Cm = v.finish_epoch()
        assert v._sync_count == syncs + 1
        for i, p in enumerate(v.votes.probs):
            err = np.abs(p.cpu().numpy() - g["%s/e%d/probs_%d" % (tag, epoch, i)]).max()
            print("case %s epoch %d cloud %d: votes differ from the float64 golden by %.3g" % (tag, epoch, i, err))
            assert err <= BOUND
        assert np.array_equal(v.last_confusion, g["%s/e%d/raw" % (tag, epoch)])
        assert Cm.dtype == np.float32 and np.array_equal(Cm, g["%s/e%d/balanced" % (tag, epoch)])
        assert np.array_equal(ious, g["%s/e%d/iou" % (tag, epoch)])
        assert int(v.confusion.sum()) == 0                                       # the next epoch starts from zero
    if tag == "A":
        projs = [dev(g["A/proj_%d" % i]) for i in range(len(sizes))]
        conf = v.reprojected_confusion(projs, [dev(a) for a in full], path=str(tmp_path / "val_preds_0_2"))
        assert np.array_equal(conf, g["A/conf_txt"])
        assert np.array_equal(np.loadtxt(str(tmp_path / "val_preds_0_2" / "conf.txt"), dtype=np.int64), g["A/conf_txt"])


# ---------------------------------------------------------------------------------------------------------------
# 2. one launch against the loop over spheres
# ---------------------------------------------------------------------------------------------------------------
def _constructed_batch(rng):
    """five spheres on tiles [0, 1, 0, 1, 0], lengths [1, 65, 64, 3, 130]; point 7 of tile 0 is listed by all three of its
    spheres (the only row of the first, the first row of the other two), point 190 by the last rows of two; the third
    sphere of tile 1 is the first, a middle and the last row of the first"""
    mid = lambda k: np.sort(rng.choice(np.arange(8, 190), size=k, replace=False))
    s0 = np.array([7])
    s2 = np.concatenate([[7], mid(62), [190]])
    s4 = np.concatenate([[7], mid(128), [190]])
    s1 = np.sort(rng.choice(100, size=65, replace=False))
    s3 = s1[[0, 30, 64]]
    lengths = np.array([1, 65, 64, 3, 130], np.int32)
    inds = np.concatenate([s0, s1, s2, s3, s4]).astype(np.int64)
    assert [len(s) for s in (s0, s1, s2, s3, s4)] == list(lengths)
    return lengths, inds, np.array([0, 1, 0, 1, 0], np.int32), [200, 100]


def _loop_and_batch(gpu, c, smooth, lengths, inds, tiles, sizes, logits, points=None, radius_mask=0.0, overlap=None, seed=3):
    from weasal_amd import tester
    dev = _dev(gpu)
    rng = np.random.default_rng(seed)
    start = [rng.random((n, c), dtype=np.float32) for n in sizes]
    loop = tester.VoteAccumulator(sizes, c, gpu, test_smooth=smooth)
    one = tester.VoteAccumulator(sizes, c, gpu, test_smooth=smooth)
    for acc in (loop, one):
        for p, s in zip(acc.probs, start):
            p.copy_(dev(s))
    pts = dev(points if points is not None else np.zeros((len(inds), 3), np.float32))
    loop.update(dev(logits), pts, lengths, dev(inds), tiles, radius_mask=radius_mask)
    one.update_batch(dev(logits), lengths, dev(inds), tiles, points0=pts, radius_mask=radius_mask, overlap=overlap)
    assert one.batch_status.cpu().tolist() == [0, 0, 0]
    return start, [p.cpu().numpy() for p in loop.probs], [p.cpu().numpy() for p in one.probs]


VAL_GRID = 1024 * 256                                              # csrc/validation.hip: ws_grid(n, 256, 1024) rows per trip


def _capped_batch(rng, in_radius=1.0):
    """eight spheres of 40 000 rows, 320 000 in all (validation_kernel strides beyond 262 144), on two tiles of 70 000
    points: every sphere lists more than half of its tile, so every pair on a tile shares thousands of points and the
    owner of a point sits up to seven spheres after its first member.  The last two spheres are on the same tile and the
    second trip of the grid starts inside the first of them: it holds rows that own their point and rows that do not.
    Points centred on the sphere, uniform in the ball of radius in_radius: the radius mask 0.7 keeps about a third"""
    nb, rows, size = 8, 40000, 70000
    tiles = np.array([0, 1, 0, 1, 0, 1, 0, 0], np.int32)
    inds = np.concatenate([np.sort(rng.choice(size, size=rows, replace=False)) for _ in range(nb)]).astype(np.int64)
    u = rng.standard_normal((nb * rows, 3))
    pts = (u / np.linalg.norm(u, axis=1, keepdims=True) * (in_radius * rng.random((nb * rows, 1)) ** (1 / 3))).astype(np.float32)
    return np.full(nb, rows, np.int32), inds, tiles, pts, [size, size]


def _assert_capped_batch(gpu, c, smooth):
    """the cases above the grid cap, by the criterion of the small ones: votes within BOUND of the loop over spheres (the
    two kernels are separate compilations and may contract smooth * p + (1 - smooth) * q differently: one ulp of a product
    per update; the identity of the bits is printed), status words zero, and the confusion of the
    same launch equal to the numpy count.  At smooth = 0.5 both products are exact whatever the contraction, one rounding
    is left, and the bits must be the loop's: an update applied out of sphere order or by two rows would change them."""
    from weasal_amd import tester, validation
    dev = _dev(gpu)
    rng = np.random.default_rng(12)
    rm = 0.7
    lengths, inds, tiles, pts, sizes = _capped_batch(rng)
    n = len(inds)
    assert n > VAL_GRID
    logits = (rng.standard_normal((n, c)) * 2).astype(np.float32)
    start, loop, one = _loop_and_batch(gpu, c, smooth, lengths, inds, tiles, sizes, logits, points=pts, radius_mask=rm)
    inside = (pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1]) + pts[:, 2] * pts[:, 2] < np.float32(rm) ** 2
    offs = np.cumsum(lengths) - lengths
    late_rows = 0
    for t, (s, a, b) in enumerate(zip(start, loop, one)):
        rows = np.concatenate([np.arange(o, o + k) for o, k, tl in zip(offs, lengths, tiles) if tl == t])
        rows = rows[inside[rows]]
        listed = np.unique(inds[rows])
        rest = np.setdiff1d(np.arange(len(s)), listed)
        assert len(rest) > 1000 and np.array_equal(b[rest], s[rest])            # untouched rows: the same bits
        assert (b[listed] != s[listed]).any(axis=1).all()
        shared = len(rows) - len(listed)
        late_rows += int((rows >= VAL_GRID).sum())
        err = np.abs(a - b).max()
        print("capped batch c=%d smooth=%g tile %d: n = %d rows, 1024 workgroups, rows visited in a second trip %d, %d points voted on, "
              "%d further listings of them, one launch against the loop: max |diff| = %.3g, bit-identical: %s"
              % (c, smooth, t, n, n - VAL_GRID, len(listed), shared, err, np.array_equal(a, b)))
        assert shared > 5000
        assert err <= BOUND
        if smooth == 0.5:
            assert np.array_equal(a, b)
    assert late_rows > 1000                                                    # unmasked rows of the second trip
    s6, s7 = (np.arange(offs[b], offs[b] + lengths[b]) for b in (6, 7))
    s6, s7 = s6[inside[s6] & (s6 >= VAL_GRID)], s7[inside[s7]]
    passed_on = int(np.isin(inds[s6], inds[s7]).sum())                          # second-trip rows whose point the last sphere owns
    assert 100 < passed_on < len(s6) - 100
    want = ref.vote_batch([s.astype(np.float64) for s in start], logits, lengths, inds, tiles, smooth=smooth, points=pts, radius_mask=rm)
    for w, b in zip(want, one):
        assert np.abs(w - b).max() <= BOUND
    # the confusion of such a launch: every row counts, masked or not, labels outside the table go to the status word
    lv = np.arange(c)
    labels = rng.integers(0, c, size=n).astype(np.int64)
    bad = rng.choice(n, size=500, replace=False)
    good = np.setdiff1d(np.arange(n), bad)
    labels[bad] = rng.choice([-1, c, c + 7], size=500)
    true_row, pred_row, _ = validation.confusion_tables(lv, [])
    acc = tester.VoteAccumulator(sizes, c, gpu, test_smooth=smooth)
    for p, s in zip(acc.probs, start):
        p.copy_(dev(s))
    conf = torch.zeros((c, c), dtype=torch.int64, device=gpu)
    acc.update_batch(dev(logits), lengths, dev(inds), tiles, points0=dev(pts), radius_mask=rm, labels=dev(labels),
                     true_row=dev(true_row), pred_row=dev(pred_row), confusion=conf)
    assert acc.batch_status.cpu().tolist() == [0, 0, 500] and (bad >= VAL_GRID).any()
    assert np.array_equal(conf.cpu().numpy(), ref.batch_confusion(logits[good], labels[good], lv, []))
    for p, b in zip(acc.probs, one):
        assert np.array_equal(p.cpu().numpy(), b)                               # the votes do not depend on the labels


@pytest.mark.parametrize("c,smooth,capped", [(4, 0.95, False), (9, 0.95, False), (4, 0.5, False), (9, 0.5, False), (4, 0.95, True),
                                             (4, 0.5, True)],
                         ids=["4-0.95", "9-0.95", "4-0.5", "9-0.5", "4-0.95-capped", "4-0.5-capped"])
def test_one_launch_equals_the_loop_over_spheres(gpu, c, smooth, capped):
    if capped:
        _assert_capped_batch(gpu, c, smooth)
        return
    rng = np.random.default_rng(11)
    lengths, inds, tiles, sizes = _constructed_batch(rng)
    logits = (rng.standard_normal((len(inds), c)) * 2).astype(np.float32)
    start, loop, one = _loop_and_batch(gpu, c, smooth, lengths, inds, tiles, sizes, logits)
    offs = np.cumsum(lengths) - lengths
    for t, (s, a, b) in enumerate(zip(start, loop, one)):
        listed = np.unique(np.concatenate([inds[o:o + n] for o, n, tl in zip(offs, lengths, tiles) if tl == t]))
        rest = np.setdiff1d(np.arange(len(s)), listed)
        assert len(rest) and np.array_equal(b[rest], s[rest])                   # untouched rows: the same bits
        assert not np.array_equal(b[listed], s[listed])
        err = np.abs(a - b).max()
        print("c=%d smooth=%g tile %d: one launch against the loop: max |diff| = %.3g, bit-identical: %s"
              % (c, smooth, t, err, np.array_equal(a, b)))
        assert err <= BOUND
    # and both are the float64 chain in sphere order
    want = ref.vote_batch([s.astype(np.float64) for s in start], logits, lengths, inds, tiles, smooth=smooth)
    for w, b in zip(want, one):
        assert np.abs(w - b).max() <= BOUND


# ---------------------------------------------------------------------------------------------------------------
# 3. / 4. spheres cut from points: centre masks, radius mask
# ---------------------------------------------------------------------------------------------------------------
def _spheres_from_points(rng, in_radius=1.0):
    """two tiles of 600 points in a 4 x 4 x 1 box; six spheres: on tile 0 two that overlap, one far from both and one that
    overlaps the first again; on tile 1 two that overlap.  Rows in ascending index order, points centred on the sphere."""
    clouds = [rng.uniform([0, 0, 0], [4, 4, 1], size=(600, 3)) for _ in range(2)]
    tiles = np.array([0, 0, 1, 0, 1, 0], np.int32)
    centres = np.array([[1.0, 1.0, 0.5], [1.8, 1.0, 0.5], [2.0, 2.0, 0.5], [3.5, 3.5, 0.5], [2.5, 2.2, 0.5], [1.2, 1.5, 0.5]])
    inds, pts, lengths = [], [], []
    for t, ctr in zip(tiles, centres):
        near = np.nonzero(((clouds[t] - ctr) ** 2).sum(axis=1) < in_radius ** 2)[0]
        inds.append(near)
        pts.append((clouds[t][near] - ctr).astype(np.float32))
        lengths.append(len(near))
    assert min(lengths) > 10
    return np.array(lengths, np.int32), np.concatenate(inds).astype(np.int64), tiles, centres, np.concatenate(pts), [600, 600]


def test_centre_masks_give_the_same_bits_as_all_pairs(gpu):
    from weasal_amd import tester, validation
    dev = _dev(gpu)
    rng = np.random.default_rng(21)
    lengths, inds, tiles, centres, _, sizes = _spheres_from_points(rng)
    logits = dev((rng.standard_normal((len(inds), 9)) * 2).astype(np.float32))
    masks = validation.overlap_from_centres(tiles, centres, 1.0)
    assert list(masks) == [0b100010, 0b100001, 0b010000, 0, 0b000100, 0b000011]  # 3 is alone; 0, 1 and 5 share; 2 and 4 share
    out = []
    for overlap in (None, masks):
        acc = tester.VoteAccumulator(sizes, 9, gpu)
        acc.update_batch(logits, lengths, dev(inds), tiles, overlap=overlap)
        acc.update_batch(logits * 0.5, lengths, dev(inds), tiles, overlap=overlap)
        assert acc.batch_status.cpu().tolist() == [0, 0, 0]
        out.append(acc.probs)
    for a, b in zip(*out):
        assert torch.equal(a, b) and float(a.abs().sum()) > 0


def test_radius_mask_moves_the_ownership(gpu):
    rng = np.random.default_rng(22)
    lengths, inds, tiles, centres, pts, sizes = _spheres_from_points(rng)
    rm = 0.7
    inside = (pts.astype(np.float64) ** 2).sum(axis=1) < rm * rm
    offs = np.cumsum(lengths) - lengths
    first, last = (inds[offs[b]:offs[b] + lengths[b]] for b in (0, 5))             # spheres 0 and 5 share points of tile 0
    in_first, in_last = (inside[offs[b]:offs[b] + lengths[b]] for b in (0, 5))
    moved = np.intersect1d(first[in_first], last[~in_last])                        # masked in the later, unmasked in the earlier
    assert len(moved) > 0
    logits = (rng.standard_normal((len(inds), 9)) * 2).astype(np.float32)
    start, loop, one = _loop_and_batch(gpu, 9, 0.95, lengths, inds, tiles, sizes, logits, points=pts, radius_mask=rm)
    for s, a, b in zip(start, loop, one):
        assert np.abs(a - b).max() <= BOUND
    assert not np.array_equal(one[0][moved], start[0][moved])                      # the earlier row did the update
    want = ref.vote_batch([s.astype(np.float64) for s in start], logits, lengths, inds, tiles, points=pts, radius_mask=rm)
    for w, b in zip(want, one):
        assert np.abs(w - b).max() <= BOUND
    masked_everywhere = np.setdiff1d(np.arange(600), np.concatenate(
        [inds[o:o + n][inside[o:o + n]] for o, n, t in zip(offs, lengths, tiles) if t == 0]))
    assert np.array_equal(one[0][masked_everywhere], start[0][masked_everywhere])


def test_a_batch_of_the_sphere_sampler(gpu):
    """what SphereSampler.sample() returns goes in as it is: lengths, tiles and centres from the state block the sampler
    has read (fields_from_sampler), ascending input_inds, no further read before finish_epoch; the centre mask names
    every pair of spheres that shares a point and gives the bits of the all-pairs mask"""
    import sampler_ref
    from test_sampler_gpu import GoldenCfg
    from weasal_amd import validation
    from weasal_amd.sampler import SphereSampler
    cfg = GoldenCfg()
    cfg.in_radius = 3.0
    clouds = [sampler_ref.slab_cloud(seed, 20000, 9.0, 1.0, 0.4) for seed in (31, 32)]
    s = SphereSampler(cfg, [(torch.from_numpy(p).to(gpu), torch.from_numpy(l).to(gpu)) for p, l in clouds], set='validation',
                      label_values=np.arange(9), seed=5, max_spheres=8, batch_limit=4000)
    out = s.sample(capacity_rows=200000)
    fields = validation.fields_from_sampler(s, out)
    lengths, tiles = fields["lengths"], np.asarray(fields["cloud_inds"])
    assert isinstance(lengths, np.ndarray) and np.array_equal(tiles, out[6].cpu().numpy()) and len(lengths) >= 3
    inds, labels = out[8].cpu().numpy(), out[2].cpu().numpy()
    offs = np.cumsum(lengths) - lengths
    masks = validation.overlap_from_centres(tiles, fields["centres"], cfg.in_radius)
    sharing = 0
    for a in range(len(lengths)):
        for b in range(a + 1, len(lengths)):
            common = tiles[a] == tiles[b] and len(np.intersect1d(inds[offs[a]:offs[a] + lengths[a]], inds[offs[b]:offs[b] + lengths[b]]))
            sharing += bool(common)
            assert not common or (int(masks[a]) >> b) & 1, "spheres %d and %d share points and the centre mask leaves them out" % (a, b)
    print("sampler batch: %d spheres, %d rows, %d pairs share points" % (len(lengths), len(inds), sharing))
    rng = np.random.default_rng(41)
    logits = (rng.standard_normal((len(inds), 9)) * 2).astype(np.float32)
    sizes = [p.shape[0] for p in s.sub_points]
    full = [torch.from_numpy(l).to(gpu) for _, l in clouds]
    by_centres, all_pairs = (validation.Validator(sizes, np.arange(9), [], full, gpu) for _ in range(2))
    by_centres.in_radius = cfg.in_radius
    syncs = s._sync_count
    for v in (by_centres, all_pairs):
        v.update(_dev(gpu)(logits), fields)
        v.finish_epoch()                                                          # raises if the indices did not ascend
    assert s._sync_count == syncs
    for a, b in zip(by_centres.votes.probs, all_pairs.votes.probs):
        assert torch.equal(a, b)
    want = ref.vote_batch([np.zeros((n, 9)) for n in sizes], logits, lengths, inds, tiles)
    for w, p in zip(want, by_centres.votes.probs):
        assert np.abs(w - p.cpu().numpy()).max() <= BOUND
    assert np.array_equal(by_centres.last_confusion, ref.batch_confusion(logits, labels, np.arange(9), []))


# ---------------------------------------------------------------------------------------------------------------
# 5. status words instead of faults
# ---------------------------------------------------------------------------------------------------------------
def _small_validator(gpu, rows=50):
    from weasal_amd import validation
    return validation.Validator([rows], [0, 1, 2, 3], [], [torch.arange(4, device=gpu).repeat(5)], gpu)


def _small_batch(rng, rows=50):
    lengths = np.array([20, 25], np.int32)
    inds = np.concatenate([np.sort(rng.choice(rows, size=int(n), replace=False)) for n in lengths]).astype(np.int64)
    logits = (rng.standard_normal((45, 4)) * 2).astype(np.float32)
    labels = rng.integers(0, 4, size=45).astype(np.int64)
    return logits, labels, lengths, inds


def _feed(v, gpu, logits, labels, lengths, inds):
    dev = _dev(gpu)
    v.update(dev(logits), {"labels": dev(labels), "lengths": lengths, "input_inds": dev(inds), "cloud_inds": [0] * len(lengths)})


def test_swapped_indices_are_counted(gpu):
    rng = np.random.default_rng(31)
    logits, labels, lengths, inds = _small_batch(rng)
    inds[[23, 24]] = inds[[24, 23]]                                                # inside the second sphere
    v = _small_validator(gpu)
    _feed(v, gpu, logits, labels, lengths, inds)
    with pytest.raises(ValueError, match=r"\b1 rows that do not ascend"):
        v.finish_epoch()
    assert int(v.status.sum()) == 0                                                # read and cleared


def test_indices_outside_the_cloud_are_counted_and_skipped(gpu):
    rng = np.random.default_rng(32)
    logits, labels, lengths, inds = _small_batch(rng)
    clean = _small_validator(gpu)
    keep = np.ones(45, bool)
    keep[[0, 44]] = False                                                          # the rows that go bad below
    _feed(clean, gpu, logits[keep], labels[keep], lengths - 1, inds[keep])
    clean.finish_epoch()
    bad = inds.copy()
    bad[0], bad[44] = -1, 50                                                       # still ascending: below and at the row count
    v = _small_validator(gpu)
    _feed(v, gpu, logits, labels, lengths, bad)
    with pytest.raises(ValueError, match=r"\b2 point ids outside their cloud"):
        v.finish_epoch()
    assert torch.equal(v.votes.probs[0], clean.votes.probs[0])                     # every other point: the clean run's vote
    assert v.last_confusion.sum() == 45                                            # the confusion needs no index


def test_labels_outside_the_table_are_counted_and_left_out(gpu):
    rng = np.random.default_rng(33)
    logits, labels, lengths, inds = _small_batch(rng)
    v = _small_validator(gpu)
    good = ref.batch_confusion(logits[2:], labels[2:], [0, 1, 2, 3], [])
    labels[0], labels[1] = 4, -1
    _feed(v, gpu, logits, labels, lengths, inds)
    with pytest.raises(ValueError, match=r"\b2 values outside the label table"):
        v.finish_epoch()
    assert np.array_equal(v.last_confusion, good)


# ---------------------------------------------------------------------------------------------------------------
# 6. edges
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb, c", [(64, 9), (1, 9), (4, 33)])
def test_sphere_counts_and_wide_rows(gpu, nb, c):
    """64 spheres of 1 to 3 rows; a single sphere; c above 16 (the kernel then keeps the vote row in 64 registers)"""
    from weasal_amd import _lib, tester
    dev = _dev(gpu)
    rng = np.random.default_rng(nb)
    lengths = rng.integers(1, 4, size=nb).astype(np.int32) if nb == 64 else np.full(nb, 70, np.int32)
    tiles = rng.integers(0, 2, size=nb).astype(np.int32)
    sizes = [90, 80]
    inds = np.concatenate([np.sort(rng.choice(sizes[t], size=int(n), replace=False)) for t, n in zip(tiles, lengths)]).astype(np.int64)
    logits = (rng.standard_normal((len(inds), c)) * 2).astype(np.float32)
    acc = tester.VoteAccumulator(sizes, c, gpu)
    before = _lib.lib().ws_launch_count()
    acc.update_batch(dev(logits), lengths, dev(inds), tiles)
    assert _lib.lib().ws_launch_count() == before + 1                              # one launch, however many spheres
    assert acc.batch_status.cpu().tolist() == [0, 0, 0]
    want = ref.vote_batch([np.zeros((n, c)) for n in sizes], logits, lengths, inds, tiles)
    for w, p in zip(want, acc.probs):
        assert np.abs(w - p.cpu().numpy()).max() <= BOUND


def test_empty_batch_and_too_many_spheres(gpu):
    from weasal_amd import _lib, tester
    dev = _dev(gpu)
    acc = tester.VoteAccumulator([10], 9, gpu)
    before = _lib.lib().ws_launch_count()
    acc.update_batch(torch.zeros((0, 9), device=gpu), np.zeros(2, np.int32), torch.zeros(0, dtype=torch.int64, device=gpu), [0, 0])
    acc.update_batch(torch.zeros((0, 9), device=gpu), [], torch.zeros(0, dtype=torch.int64, device=gpu), [])
    assert _lib.lib().ws_launch_count() == before and float(acc.probs[0].abs().sum()) == 0
    with pytest.raises(_lib.WeasalHipError, match="at most 64 spheres"):
        acc.update_batch(torch.zeros((65, 9), device=gpu), np.ones(65, np.int32), dev(np.zeros(65, np.int64)), np.zeros(65, np.int32))
    with pytest.raises(ValueError, match="blocking read"):
        acc.update_batch(torch.zeros((2, 9), device=gpu), dev(np.array([2], np.int32)), dev(np.zeros(2, np.int64)), [0])


# ---------------------------------------------------------------------------------------------------------------
# 7. one blocking read per epoch
# ---------------------------------------------------------------------------------------------------------------
def test_run_epoch_reads_once(gpu):
    from weasal_amd import validation
    g, dev = golden("g19_validation.npz"), _dev(gpu)

    class Batch:
        pass

    batches = []
    for k in range(3):
        key, b = "B/e0/b%d/" % k, Batch()
        b.logits, b.labels, b.input_inds = dev(g[key + "logits"]), dev(g[key + "labels"]), dev(g[key + "inds"])
        b.lengths, b.cloud_inds = [torch.from_numpy(g[key + "lengths"])], torch.from_numpy(g[key + "clouds"])    # host, per layer
        batches.append(b)

    class Net:
        calls = []

        def eval(self):
            self.calls.append("eval")

        def train(self):
            self.calls.append("train")

        def __call__(self, batch, config):
            self.calls.append("forward")
            return batch.logits, None, None                                      # the weak-label triple

    v = validation.Validator(g["B/cloud_sizes"], g["B/label_values"], [], [dev(g["B/full_labels_0"])], gpu)
    net, before = Net(), v._sync_count
    ious, Cm = v.run_epoch(net, batches, None)
    assert v._sync_count == before + 1
    assert net.calls == ["eval", "forward", "forward", "forward", "train"]
    assert np.array_equal(ious, g["B/e0/iou"]) and np.array_equal(Cm, g["B/e0/balanced"])
    v.run_epoch(lambda batch, config: batch.logits, batches, None)                # any callable
    assert v._sync_count == before + 2
