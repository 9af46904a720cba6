"""GPU: the count-only calibration.  ws_radius_neighbors_histogram against np.bincount of brute-force counts
(oracle/neighbors_ref), pyramid.neighbor_histograms against the older route (an un-limited build_batch counted by
NeighborhoodCalibrator) under the same np.random seed, and calibration.calibrate driving the real SphereSampler.
Everything is integers: equality, no tolerance."""
import numpy as np
import pytest
import torch

from conftest import golden, sphere
from oracle import neighbors_ref as R
from weasal_amd import _lib, calibration, ops, pyramid, synthetic

HIST_MAX = _lib.ABI.constants["WS_NB_HIST_MAX"]
SEED = 11


# ------------------------------------------------------------------------------------------------------------------
# one search
# ------------------------------------------------------------------------------------------------------------------
def _sets():
    rng = np.random.default_rng(21)
    cloud = sphere(rng, 5000, 2.5)
    other = np.concatenate([sphere(rng, 200, 1.0), sphere(rng, 30, 1.0, center=(9, 9, 9))])
    return {
        # name: (queries, supports, q_lens, s_lens, radius); queries None = the supports tensor itself (walked in cell order)
        "one_query": (cloud[:1].copy(), cloud[:300].copy(), [1], [300], 0.9),
        "empty_element": (np.concatenate([other[:40], other[200:]]), other[:200].copy(), [40, 30], [200, 0], 0.4),
        "self_5000": (None, cloud, [3000, 2000], [3000, 2000], 0.4),
        "cross_5000": (cloud[::-1].copy(), cloud, [2000, 3000], [3000, 2000], 0.4),
    }


@pytest.fixture(scope="module")
def searches():
    """name -> (set, brute-force counts), computed once and never changed"""
    out = {}
    for name, (q, s, ql, sl, r) in _sets().items():
        _, counts = R.brute_keys(s if q is None else q, s, ql, sl, r)
        out[name] = ((q, s, ql, sl, r), counts)
    return out


def _run(dev, data, hist_n, hist=None):
    q, s, ql, sl, r = data
    s_d = torch.from_numpy(s).to(dev)
    q_d = s_d if q is None else torch.from_numpy(q).to(dev)
    if hist is None:
        hist = torch.zeros(hist_n, dtype=torch.int64, device=dev)
    return ops.radius_neighbors_histogram(q_d, s_d, ql, sl, r, hist)


def _want(counts, hist_n):
    return np.bincount(counts, minlength=hist_n)[:hist_n]


@pytest.mark.gpu
@pytest.mark.parametrize("name, hist_n", [("one_query", 512), ("empty_element", 64), ("self_5000", 64), ("cross_5000", 64),
                                          ("self_5000", 16), ("cross_5000", 1), ("empty_element", 1), ("self_5000", HIST_MAX),
                                          ("one_query", HIST_MAX)])
def test_histogram_equals_bincount_of_brute_force_counts(gpu, searches, name, hist_n):
    data, counts = searches[name]
    got = _run(gpu, data, hist_n).cpu().numpy()
    want = _want(counts, hist_n)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    if name == "one_query":
        assert got.sum() == 1 and counts[0] > 1
    if name == "empty_element":
        assert (counts[40:] == 0).all() and want[0] >= 30          # the queries of the element without supports: bin 0
    if name.endswith("5000") and hist_n == 64:
        assert counts.max() < 64 and got.sum() == 5000 and want.max() > 64      # a bin holds more than any one workgroup's 16 queries
    if hist_n == 16:
        assert counts.max() >= 16 and 0 < got.sum() < 5000         # counts of hist_n and above are dropped, the rest exact
    if hist_n == 1 and name == "cross_5000":
        assert got[0] == (counts == 0).sum()


@pytest.mark.gpu
def test_the_entry_adds_to_hist(gpu, searches):
    (data_a, counts_a), (data_b, counts_b) = searches["self_5000"], searches["empty_element"]
    hist = _run(gpu, data_a, 48)
    first = hist.clone()
    _run(gpu, data_b, 48, hist)
    _run(gpu, data_a, 48, hist)
    assert np.array_equal(first.cpu().numpy(), _want(counts_a, 48))
    assert np.array_equal(hist.cpu().numpy(), 2 * _want(counts_a, 48) + _want(counts_b, 48))
    with pytest.raises(_lib.WeasalHipError, match="status 2"):
        _run(gpu, data_b, HIST_MAX + 1)
    with pytest.raises(ValueError):
        ops.radius_neighbors_histogram(first.float().view(-1, 3), first.float().view(-1, 3), [16], [16], 1.0, hist.int())


# ------------------------------------------------------------------------------------------------------------------
# the count-only pyramid against the older route
# ------------------------------------------------------------------------------------------------------------------
BATCHES = {"A": (3, 2, 1500), "B": (5, 3, 600)}
# figures of the CPU oracle (oracle/pyramid_ref.segmentation_inputs(..., ()) under np.random.seed(11), orientations on)
ORACLE_MAX = {"A": [37, 70, 81, 30, 8], "B": [20, 53, 80, 30, 8]}
ORACLE_DROPPED_34 = {"A": [12, 1011, 235, 0, 0], "B": [0, 498, 246, 0, 0]}


def _config(variant):
    from test_oracle_cpu_kpconv import _small_config
    cfg = _small_config()
    if variant == "deformable":               # the later layers search at the deformable radius
        arch = list(cfg.architecture)
        for i in (5, 6, 7, 9):
            arch[i] = arch[i].replace('resnetb', 'resnetb_deformable')
        type(cfg).architecture = arch
        cfg = type(cfg)()
        cfg.deform_radius = 4.0
    if variant == "radius1":
        cfg.deform_radius = 1.0
    return cfg


@pytest.fixture(scope="module")
def inputs(gpu):
    out = {}
    for name, (seed, spheres, points) in BATCHES.items():
        p, f, l, le = synthetic.make_inputs(seed, spheres, points, 2.5, 4)
        out[name] = (torch.from_numpy(p).to(gpu), torch.from_numpy(f).to(gpu), torch.from_numpy(l).to(gpu), le)
    return out


def _older_route(cfg, batch_in, orient, hist_n):
    p, f, l, le = batch_in
    np.random.seed(SEED)
    batch = pyramid.build_batch(cfg, p, f, l, le, (), random_grid_orient=orient)
    cal = calibration.NeighborhoodCalibrator(cfg)
    cal.hist_n = hist_n
    cal.update(batch)
    return cal.hists.cpu().numpy(), [np.asarray(a) for a in batch.lengths_host], np.random.rand(), batch


@pytest.mark.gpu
@pytest.mark.parametrize("orient", [True, False])
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("variant", ["base", "radius1", "hist16", "deformable"])
def test_neighbor_histograms_equal_the_older_route(gpu, inputs, variant, name, orient):
    cfg = _config(variant)
    hist_n = 16 if variant == "hist16" else calibration.histogram_size(cfg)
    assert hist_n == {"base": 1437, "radius1": 34, "hist16": 16, "deformable": 524}[variant]
    want, want_lens, want_rand, batch = _older_route(cfg, inputs[name], orient, hist_n)
    hists = torch.zeros((cfg.num_layers, hist_n), dtype=torch.int64, device=gpu)
    np.random.seed(SEED)
    lens = pyramid.neighbor_histograms(cfg, inputs[name][0], inputs[name][3], hists, random_grid_orient=orient)
    got_rand = np.random.rand()
    got = hists.cpu().numpy()
    assert len(lens) == len(want_lens) == 5
    for a, b in zip(lens, want_lens):
        assert a.dtype == np.int32 and np.array_equal(a, b)
    assert got_rand == want_rand                                    # the same draws were consumed
    assert np.array_equal(got, want)
    sizes = np.array([int(a.sum()) for a in lens])
    widest = [int((m < m.shape[0]).sum(1).max()) for m in batch.neighbors]
    if variant == "base":
        assert np.array_equal(got.sum(1), sizes)                    # nothing dropped: one entry per point and layer
        if orient:
            assert widest == ORACLE_MAX[name]
    if variant == "radius1" and orient:
        assert list(sizes - got.sum(1)) == ORACLE_DROPPED_34[name]
    if variant == "hist16":
        lim = list(calibration.limits_from_histograms(got))
        assert lim == ([15, 0, 0, 0, 8] if name == "A" else [12, 15, 0, 0, 8])     # whole layers vanish: limit 0
    if variant == "deformable":
        base = pyramid._schedule(_config("base"), ())
        mine = pyramid._schedule(cfg, ())
        assert [m["r_conv"] > b["r_conv"] for m, b in zip(mine, base)] == [False, False, True, True, True]
        assert widest[2] > ORACLE_MAX[name][2]


@pytest.mark.gpu
def test_the_same_batch_twice_gives_identical_bytes(gpu, inputs):
    cfg = _config("base")
    runs = []
    for _ in range(2):
        cal = calibration.DeviceCalibrator(cfg, gpu)
        for name in ("A", "B", "A"):
            cal.update(inputs[name][0], inputs[name][3], rng=np.random.RandomState(4))
        runs.append(cal.hists.cpu().numpy().tobytes())
        assert cal.hists.shape == (5, cal.hist_n) and cal.hist_n == 1437
    assert runs[0] == runs[1]


@pytest.mark.gpu
def test_an_update_allocates_no_matrix(gpu, inputs):
    """The device memory an update takes is its scratch, two copies of the level-0 points.  The bound on the rise is
    scratch + 64 KiB of allocator rounding -- tighter than the scratch + 1 MiB the feature was specified with, because that
    figure is not below the un-limited level-0 matrix of a 3000-point batch (n0 * 37 * 8 = 888 000 bytes), which the
    bound must be for the test to tell the two routes apart."""
    cfg = _config("base")
    p, _, _, le = inputs["A"]
    n0 = int(p.shape[0])
    cal = calibration.DeviceCalibrator(cfg, gpu)
    cal.update(p, le, rng=np.random.RandomState(1))                  # warm-up: workspaces, library state
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(gpu)
    before = torch.cuda.max_memory_allocated(gpu)
    cal.update(p, le, rng=np.random.RandomState(1))
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(gpu) - before
    scratch = int(_lib.lib().ws_pyramid_histograms_scratch_bytes(n0))
    bound = scratch + (64 << 10)
    print("rise %d bytes, scratch %d, bound %d, level-0 matrix %d" % (rise, scratch, bound, n0 * 37 * 8))
    assert bound <= scratch + (1 << 20)
    assert bound < n0 * 37 * 8
    assert rise <= bound


# ------------------------------------------------------------------------------------------------------------------
# the routine with the real sampler
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_calibrate_with_the_sphere_sampler(gpu):
    from test_sampler_cpu import golden_scene
    from test_sampler_gpu import GoldenCfg
    from weasal_amd.sampler import SphereSampler
    g = golden("g15_sampler.npz")
    clouds, _, _ = golden_scene(g)
    base = _config("base")

    class Cfg(GoldenCfg, type(base)):
        pass
    cfg = Cfg()
    cfg.in_radius, cfg.batch_num = float(g['in_radius']), 4
    cfg.first_subsampling_dl = float(g['dl'])                        # the clouds' own cell: level 0 searches at 1 m in 6.5 m spheres
    cfg.deform_radius = 4.0
    sampler = SphereSampler(cfg, [(torch.from_numpy(p).to(gpu), torch.from_numpy(l).to(gpu)) for p, l in clouds],
                            label_values=g['label_values'], seed=3, max_spheres=int(g['max_spheres']))
    kept = []

    def keep(batch):      # called before the batch is counted: the stream's state is the one its orientations are drawn from
        kept.append((batch[0].clone(), np.array(batch[3]), sampler.rng.get_state()))
    cal = calibration.DeviceCalibrator(cfg, gpu)
    with pytest.raises(calibration.CalibrationError) as e:
        calibration.calibrate(sampler, cfg, sample_batches=40, n_per_epoch=20, on_batch=keep, calibrator=cal)
    assert len(kept) == 60 and len(e.value.b) == 60                  # 60 batches cannot converge
    ctl = calibration.BatchLimitController(target_b=4, batch_limit=1.0)
    assert e.value.batch_limit == [int(ctl.update(len(le))) for _, le, _ in kept]
    assert e.value.b == [len(le) for _, le, _ in kept] and e.value.points_per_batch == [int(p.shape[0]) for p, _, _ in kept]
    assert sampler.batch_limit == ctl.batch_limit and max(e.value.b) > 1
    # the summed histograms against the older route over the kept batches
    older = calibration.NeighborhoodCalibrator(cfg)
    rng = np.random.RandomState()
    for p, le, state in kept:
        rng.set_state(state)
        f = torch.ones((p.shape[0], 1), device=gpu)
        older.update(pyramid.build_batch(cfg, p, f, torch.zeros(p.shape[0], dtype=torch.int64, device=gpu), le, (), rng=rng))
    got, want = cal.hists.cpu().numpy(), older.hists.cpu().numpy()
    assert np.array_equal(got, want) and want[0].sum() == sum(e.value.points_per_batch)
    assert (want[:, -1] == 0).all()                                  # nothing was dropped at this hist_n
