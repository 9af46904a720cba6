"""Voting tester / re-projection / potentials against tests/golden/g11_tester.npz: confusion
matrices and IoUs from the reference's own utils/metrics.py, votes / projection / potentials from the reference's tester
arithmetic with the reference's own KDTree library calls (tests/golden/make_golden_tester.py).  CPU part: the numpy
metrics of weasal_amd.tester and the oracle restatement; GPU part: the HIP kernels and the K1-based projection."""
import numpy as np
import pytest
import torch

from conftest import golden


def test_metrics_match_the_reference_functions():
    from weasal_amd.tester import IoU_from_confusions, fast_confusion
    g = golden("g11_tester.npz")
    lv = np.arange(9).astype(np.int64)
    assert np.array_equal(fast_confusion(g["sub_labels"], g["preds_sub"], lv), g["conf_sub"])
    assert np.array_equal(fast_confusion(g["full_labels"], g["preds_full"], lv), g["conf_full"])
    assert np.array_equal(fast_confusion(g["t2"], g["p2"], g["lv2"]), g["conf2"])        # label map through an ignored gap
    assert np.allclose(IoU_from_confusions(g["conf_full"]), g["iou_full"], rtol=0, atol=0)
    Cs = g["conf_sub"].astype(np.float32)
    Cs *= np.expand_dims(g["val_prop"] / (np.sum(Cs, axis=1) + 1e-6), 1)
    assert np.array_equal(IoU_from_confusions(Cs), g["iou_sub"])
    with pytest.raises(ValueError):
        fast_confusion(np.zeros(3, np.float32), np.zeros(3, np.int32))


def test_oracle_restatement_reproduces_the_fixture():
    from oracle import tester_ref
    g = golden("g11_tester.npz")
    probs = [np.zeros_like(g["test_probs"])]
    for i in range(3):
        probs = tester_ref.vote_update(probs, g["logits_%d" % i], g["points_%d" % i], g["lengths_%d" % i], g["inds_%d" % i],
                                       np.array([0, 0]), float(g["in_radius"]), 0.7, 0.95)
    assert np.array_equal(probs[0], g["test_probs"])


@pytest.mark.gpu
def test_projection_votes_confusion_potentials_on_the_gpu(gpu):
    from weasal_amd import tester
    g = golden("g11_tester.npz")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    # ---- nearest-neighbour projection = column 0 of the K1 search
    proj = tester.nearest_projection(dev(g["full"]), dev(g["sub"]), float(g["dl"]) * 3 ** 0.5)
    got = proj.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == g["proj"].shape
    diff = np.nonzero(got != g["proj"])[0]
    if len(diff):        # only where two sub-cloud points are equally near in f32 (the tree decides in f64)
        full, sub = g["full"].astype(np.float64), g["sub"].astype(np.float64)
        d_got = ((full[diff] - sub[got[diff]]) ** 2).sum(1)
        d_ref = ((full[diff] - sub[g["proj"][diff]]) ** 2).sum(1)
        assert len(diff) < 1e-3 * len(got) and np.all(np.abs(d_got - d_ref) <= 1e-6 * d_ref)
    # ---- votes: softmax + radius mask + smoothing, sphere by sphere
    votes = tester.VoteAccumulator([g["sub"].shape[0]], 9, gpu, test_smooth=0.95)
    for i in range(3):
        votes.update(dev(g["logits_%d" % i]), dev(g["points_%d" % i]), g["lengths_%d" % i], dev(g["inds_%d" % i]),
                     np.array([0, 0]), radius_mask=0.7 * float(g["in_radius"]))
    p = votes.probs[0].cpu().numpy()
    assert np.abs(p - g["test_probs"]).max() < 2e-6                      # expf vs numpy's exp: last-ulp differences
    untouched = ~np.isin(np.arange(p.shape[0]), np.concatenate([g["inds_%d" % i] for i in range(3)]))
    assert np.all(p[untouched] == 0)
    # ---- predictions and confusions (sub cloud, then re-projected on the full cloud), from the reference's votes
    votes.probs[0].copy_(dev(g["test_probs"]))
    preds, conf = votes.predictions(0, labels=dev(g["sub_labels"]))
    assert np.array_equal(preds.cpu().numpy(), g["preds_sub"]) and np.array_equal(conf.cpu().numpy(), g["conf_sub"])
    preds, conf = votes.predictions(0, proj=dev(g["proj"]), labels=dev(g["full_labels"]))
    assert np.array_equal(preds.cpu().numpy(), g["preds_full"]) and np.array_equal(conf.cpu().numpy(), g["conf_full"])
    assert np.array_equal(tester.IoU_from_confusions(conf.cpu().numpy()), g["iou_full"])
    # ---- potentials: float64 Tukey update + arg-min
    pots = dev(g["pots0"]).clone()
    mn, am = tester.update_potentials(dev(g["pot_points"]), pots, g["center"], float(g["in_radius"]))
    assert np.abs(pots.cpu().numpy() - g["pots1"]).max() <= 4e-16
    assert int(am.item()) == int(g["argmin1"]) and float(mn.item()) == float(pots.cpu().numpy().min())


@pytest.mark.gpu
def test_ignored_labels_and_unvisited_points(gpu):
    """tests/golden/g13_tester_ignored.npz (the reference tester's zero-column insertion and row / column deletion,
    tester_PseudoLabel.py:228-250, 287-307): an ignored label in front of the valid ones (DALES: 0 = unclassified), or in the
    middle; sub-cloud points no sphere ever voted on"""
    from weasal_amd import tester
    g, s = golden("g11_tester.npz"), golden("g13_tester_ignored.npz")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    votes = tester.VoteAccumulator([g["sub"].shape[0]], 9, gpu, test_smooth=0.95)
    votes.probs[0].copy_(dev(g["test_probs"]))
    assert int((g["test_probs"].sum(1) == 0).sum()) > 0
    for tag in ("first", "middle"):
        lv, ign = s[tag + "/label_values"], s[tag + "/ignored"]
        for name, proj in (("sub", None), ("full", dev(g["proj"]))):
            preds, conf = votes.predictions(0, proj=proj, labels=dev(s["%s/%s/targets" % (tag, name)]), label_values=lv,
                                            ignored_labels=ign)
            assert np.array_equal(preds.cpu().numpy(), s["%s/%s/preds" % (tag, name)]), (tag, name)
            assert np.array_equal(conf.cpu().numpy(), s["%s/%s/conf" % (tag, name)]), (tag, name)
            assert np.array_equal(tester.IoU_from_confusions(conf.cpu().numpy()), s["%s/%s/iou" % (tag, name)])


# ---------------------------------------------------------------------------------------------------------------
# above the grid caps of csrc/tester.hip: argmin_partial_kernel and project_confusion_kernel get at most 1024 workgroups
# of 256 threads and stride beyond 262 144 items; argmin_final_kernel strides beyond 256 partials (65 536 items)
# ---------------------------------------------------------------------------------------------------------------
TESTER_GRID = 1024 * 256


def _tukey_reference(pot_points, pots, centre, radius):
    """the Tukey update of tests/sampler_ref.py (RefSampler.batch), float64, on a copy"""
    from sklearn.neighbors import KDTree
    out = np.array(pots, dtype=np.float64)
    inds, dists = KDTree(np.asarray(pot_points), leaf_size=10).query_radius(np.asarray(centre, np.float64).reshape(1, 3), r=radius,
                                                                            return_distance=True)
    d2s = np.square(dists[0])
    tukeys = np.square(1 - d2s / np.square(radius))
    tukeys[d2s > np.square(radius)] = 0
    out[inds[0]] += tukeys
    return out, inds[0]


@pytest.fixture(scope="module")
def capped_pot_points():
    import sampler_capped_scene as cs
    return cs.scene().pot_points[0]


@pytest.mark.gpu
@pytest.mark.parametrize("start", ["random", "constant", "last", "one_point", "whole_cloud"])
def test_potentials_update_above_the_grid_caps(gpu, capped_pot_points, start):
    """start potentials as the sampler draws them (below 1e-3), so the updated ones stay O(1) and the bound of
    test_projection_votes_confusion_potentials_on_the_gpu, 4e-16 absolute, applies as it stands.
    random: no ties; constant: the arg-min is the first index outside the ball, among equal values in every workgroup and
    trip; last: a unique minimum at index p - 1 (the last item of the second trip); one_point: n = 1; whole_cloud: a ball
    that holds every point, so every potential changes."""
    from weasal_amd import tester
    pp = capped_pot_points
    p = len(pp)
    assert p > TESTER_GRID
    radius = 1.0
    centre = pp[0].astype(np.float64) + np.array([0.03, -0.02, 0.01])
    rs = np.random.RandomState(4140)
    pots0 = rs.rand(p) * 1e-3
    if start in ("constant", "last"):
        pots0 = np.full(p, 5e-4)
    if start == "last":
        pots0[p - 1] = 1e-4
    if start == "one_point":
        pp, pots0 = pp[:1], pots0[:1]
    if start == "whole_cloud":
        centre, radius = np.array([0.5, -0.25, 0.0]), 40.0
    want, ball = _tukey_reference(pp, pots0, centre, radius)
    n = len(pp)
    if start == "whole_cloud":
        assert len(ball) == n
    elif start == "one_point":
        assert len(ball) == 1
    else:
        assert 100 < len(ball) < n // 100 and 0 in ball and n - 1 not in ball
    pots = torch.from_numpy(pots0).to(gpu)
    mn, am = tester.update_potentials(torch.from_numpy(pp).to(gpu), pots, centre, radius)
    got = pots.cpu().numpy()
    err = np.abs(got - want).max()
    print("potentials %s: n = %d, %d workgroups, %d partials for the final step, items visited in a second trip %d, "
          "%d in the ball, max |diff| = %.3g" % (start, n, min(-(-n // 256), 1024), min(-(-n // 256), 1024),
                                                 max(n - TESTER_GRID, 0), len(ball), err))
    assert err <= 4e-16
    outside = np.setdiff1d(np.arange(n), ball)
    assert np.array_equal(got[outside], pots0[outside])                              # untouched: the same bits
    assert int(am.item()) == int(np.argmin(want)) == int(np.argmin(got))
    assert float(mn.item()) == float(got.min())
    if start == "constant":
        assert int(am.item()) == outside[0] and (got[outside] == 5e-4).all()
    if start == "last":
        assert int(am.item()) == n - 1 >= TESTER_GRID


@pytest.mark.gpu
def test_predictions_and_confusion_above_the_grid_cap(gpu):
    """300 000 rows re-projected onto a vote table of 5 000 rows, c = 9: project_confusion_kernel strides.  Labels outside
    the table are not counted; a row of all-zero votes and a row with two equal maxima take the first maximum."""
    from weasal_amd import tester
    rows, m, c = 5000, 300000, 9
    assert m > TESTER_GRID
    rs = np.random.RandomState(4150)
    probs = rs.rand(rows, c).astype(np.float32)
    probs[rs.choice(rows, size=400, replace=False)] = 0                             # never voted on
    tied = rs.choice(rows, size=400, replace=False)
    probs[tied, 6] = probs[tied, 2] = probs[tied].max(axis=1)                       # two equal maxima: column 2 wins
    proj = rs.randint(0, rows, size=m).astype(np.int32)
    labels = rs.randint(0, c, size=m).astype(np.int32)
    outside = rs.choice(m - 1, size=3000, replace=False)
    labels[outside] = rs.choice([9, 11, 40], size=3000)
    labels[m - 1], proj[m - 1] = 3, rows - 1                                        # the last row of the second trip is counted
    votes = tester.VoteAccumulator([rows], c, gpu)
    votes.probs[0].copy_(torch.from_numpy(probs))
    preds, conf = votes.predictions(0, proj=torch.from_numpy(proj).to(gpu), labels=torch.from_numpy(labels).to(gpu))
    preds, conf = preds.cpu().numpy(), conf.cpu().numpy()
    want = np.argmax(probs[proj], axis=1)
    assert preds.dtype == np.int32 and np.array_equal(preds, want)
    zero, two = (probs[proj] == 0).all(axis=1), np.isin(proj, tied)
    assert zero[TESTER_GRID:].any() and two[TESTER_GRID:].any() and (want[zero] == 0).all() and (want[two & ~zero] <= 2).all()
    counted = labels < c
    assert counted.sum() == m - 3000 and (~counted[TESTER_GRID:]).any()
    assert conf.dtype == np.int64 and np.array_equal(conf, tester.fast_confusion(labels[counted], want[counted].astype(np.int32),
                                                                                   np.arange(c)))
    assert conf.sum() == m - 3000
    # the sub-cloud path (no projection) on the same number of rows
    big = tester.VoteAccumulator([m], c, gpu)
    big.probs[0].copy_(torch.from_numpy(probs[proj]))
    preds2, conf2 = big.predictions(0, labels=torch.from_numpy(labels).to(gpu))
    assert np.array_equal(preds2.cpu().numpy(), want) and np.array_equal(conf2.cpu().numpy(), conf)
    print("project_confusion: m = %d rows, 1024 workgroups, rows visited in a second trip %d (%d of them all-zero, %d tied, "
          "%d with a label outside the table)" % (m, m - TESTER_GRID, zero[TESTER_GRID:].sum(), two[TESTER_GRID:].sum(),
                                                  (~counted[TESTER_GRID:]).sum()))
