"""GPU: weasal_amd.sampler.SphereSampler (ws_sampler_batch, csrc/sampler.hip) against golden g15_sampler.npz and against
tests/sampler_ref.py run on the CPU in the same test.  Every pinned expression is specified to the rounding, so integers
are compared for equality and floats bit for bit: no tolerance anywhere but in the statistics of the noise generator."""
import numpy as np
import pytest
import torch

from conftest import golden

import sampler_ref
from test_sampler_cpu import DRAW_DTYPE, assert_batch_equals_golden, golden_draws, golden_scene

NAMES = ('points', 'features', 'labels', 'lengths', 'scales', 'rots', 'cloud_inds', 'point_inds', 'input_inds')


class GoldenCfg:
    """the configuration the golden was made with (make_golden_sampler.py)"""
    in_features_dim = 3
    augment_rotation = 'vertical'
    augment_scale_anisotropic = True
    augment_scale_min = 0.9
    augment_scale_max = 1.1
    augment_symmetries = [True, False, False]
    augment_noise = 0.0
    batch_num = 4


def as_numpy(out):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in zip(NAMES, out)}


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same_batch(a, b):
    for k in NAMES:
        assert bits_equal(a[k], b[k]), k


def make_sampler(g, scene, dev, **kw):
    from weasal_amd.sampler import SphereSampler
    clouds, pot_points, pots0 = scene
    cfg = GoldenCfg()
    cfg.in_radius = float(g['in_radius'])
    kw.setdefault('max_spheres', int(g['max_spheres']))
    kw.setdefault('seed', 3)
    s = SphereSampler(cfg, [(torch.from_numpy(p).to(dev), torch.from_numpy(l).to(dev)) for p, l in clouds],
                      label_values=g['label_values'], batch_limit=int(g['batch_limit']), **kw)
    for i, pp in enumerate(pot_points):                       # the HIP grid subsampling equals the CPU oracle's (K2)
        assert bits_equal(s.pot_points[i].cpu().numpy(), pp)
    s.set_potentials(pots0)
    return s


@pytest.fixture(scope="module")
def scene():
    g = golden("g15_sampler.npz")
    return g, golden_scene(g)


@pytest.mark.gpu
def test_six_chained_batches_equal_the_golden_and_the_cpu_restatement(gpu, scene):
    g, sc = scene
    s = make_sampler(g, sc, gpu)
    ref = sampler_ref.RefSampler(sc[0], sc[1], sc[2], float(g['in_radius']))
    for b in range(6):
        d = golden_draws(g, 'b%d' % b)
        got = as_numpy(s.sample(draws=d))
        pots = [p.cpu().numpy() for p in s.potentials]
        assert_batch_equals_golden(g, 'b%d' % b, got, pots)
        want = ref.batch(d, s.max_spheres, s.batch_limit, fd=3, lut=g['lut'])
        assert got['labels'].dtype == np.int64 and got['input_inds'].dtype == np.int64 and got['lengths'].dtype == np.int32
        for k in ('lengths', 'cloud_inds', 'point_inds', 'input_inds', 'labels'):
            assert np.array_equal(got[k], want[k]), (b, k)
        for k in ('points', 'features', 'scales', 'rots'):
            assert bits_equal(got[k], want[k]), (b, k)
        for i in range(2):
            assert bits_equal(pots[i], ref.potentials[i]), (b, i)
        assert bits_equal(s.last_centres, want['centres'])
        assert np.array_equal(s.lengths_dev.cpu().numpy(), got['lengths'])
        limit = int(s.batch_limit)
        assert np.sum(got['lengths'][:-1]) <= limit < np.sum(got['lengths'])            # the stop rule
    assert s.failed == 0 and s._sync_count == 6


@pytest.mark.gpu
def test_dropped_sphere_counts_updates_potentials_and_the_batch_goes_on(gpu, scene):
    g, sc = scene
    s = make_sampler(g, sc, gpu)
    d = golden_draws(g, 'drop')
    got = as_numpy(s.sample(draws=d))
    pots = [p.cpu().numpy() for p in s.potentials]
    assert_batch_equals_golden(g, 'drop', got, pots)
    assert s.last_failed == 1 and s.failed == 1 and len(got['lengths']) >= 2
    head, slots = s.last_state
    assert slots[0, 4] == -1 and slots[0, 0] < 2 and head['attempts'] == len(got['lengths']) + 1
    # the dropped sphere's potentials did take the update: the cloud's potentials differ from a run without slot 0
    ref = sampler_ref.RefSampler(sc[0], sc[1], sc[2], float(g['in_radius']))
    want = ref.batch(d, s.max_spheres, s.batch_limit, fd=3, lut=g['lut'])
    for i in range(2):
        assert bits_equal(pots[i], ref.potentials[i])
    assert want['n_fail'] == 1 and bits_equal(got['points'], want['points'])


@pytest.mark.gpu
def test_stop_rule_cap_and_capacity_retry(gpu, scene):
    g, sc = scene
    d = golden_draws(g, 'b0')
    roomy = make_sampler(g, sc, gpu)
    want = as_numpy(roomy.sample(draws=d, capacity_rows=100000))
    assert roomy._sync_count == 1
    limit = int(roomy.batch_limit)
    assert np.sum(want['lengths'][:-1]) <= limit < np.sum(want['lengths'])
    want_pots = [p.cpu().numpy() for p in roomy.potentials]
    for cap in (100, 3000, int(np.sum(want['lengths'])) - 1):           # the first, the second, the last sphere does not fit
        s = make_sampler(g, sc, gpu)
        got = as_numpy(s.sample(draws=d, capacity_rows=cap))
        assert s._sync_count >= 2, "the small buffer must have been noticed"
        assert_same_batch(got, want)
        for p, w in zip(s.potentials, want_pots):
            assert bits_equal(p.cpu().numpy(), w)
        assert s.seq == roomy.seq
    # max_spheres is a hard cap
    s = make_sampler(g, sc, gpu, max_spheres=2)
    s.batch_limit = 10 ** 9
    got = as_numpy(s.sample(draws=d[:2]))
    assert len(got['lengths']) == 2 and np.array_equal(got['lengths'], want['lengths'][:2])
    assert bits_equal(got['points'], want['points'][:int(np.sum(got['lengths']))])
    with pytest.raises(ValueError):
        from weasal_amd.sampler import SphereSampler
        SphereSampler(s.config, [(s.sub_points[0], s.sub_labels[0])], max_spheres=65)
    bad = GoldenCfg()
    bad.in_radius, bad.in_features_dim = 6.5, 4
    with pytest.raises(ValueError, match='Only accepted input dimensions are 1 and 3'):
        from weasal_amd.sampler import SphereSampler
        SphereSampler(bad, [(s.sub_points[0], s.sub_labels[0])])


@pytest.mark.gpu
def test_noise_is_a_pure_function_of_its_key_and_is_standard_normal(gpu, scene):
    g, sc = scene
    d8 = golden_draws(g, 'b0')
    d16 = np.zeros(16, DRAW_DTYPE)
    d16[:8], d16[8:] = d8, d8
    sigma = 0.05

    def run(max_spheres, draws, seq=0, noise=sigma):
        s = make_sampler(g, sc, gpu, max_spheres=max_spheres, seed=7)
        s.seq = seq
        return as_numpy(s.sample(draws=draws, augment_noise=noise))
    a, b, c = run(8, d8), run(8, d8), run(16, d16)
    assert_same_batch(a, b)                                    # same (seed, seq): same bits
    assert_same_batch(a, c)                                    # whatever the length of the chain
    other = run(8, d8, seq=100)
    assert bits_equal(a['input_inds'], other['input_inds']) and not bits_equal(a['points'], other['points'])
    zero = run(8, d8, noise=0.0)
    assert bits_equal(a['input_inds'], zero['input_inds'])
    diff = (a['points'].astype(np.float64) - zero['points'].astype(np.float64)).reshape(-1)
    m = diff.size
    assert m >= 30000 and np.isfinite(a['points']).all() and np.isfinite(a['features']).all()
    mean, std = diff.mean(), diff.std()
    print("noise: m = %d, mean = %.3e (5 s.e. = %.3e), std = %.6f (sigma = %g, 5 s.e. = %.3e)"
          % (m, mean, 5 * sigma / np.sqrt(m), std, sigma, 5 * sigma / np.sqrt(2 * m)))
    assert abs(mean) < 5 * sigma / np.sqrt(m)                   # standard error of the mean of m N(0, sigma^2) values
    assert abs(std - sigma) < 5 * sigma / np.sqrt(2 * m)        # standard error of their standard deviation
    # the height feature follows the noisy point (DALES_PseudoLabel.py:389)
    assert bits_equal(a['features'][:, 2], a['points'][:, 2]) and (a['features'][:, 0] == 1).all()


@pytest.mark.gpu
def test_one_synchronisation_and_a_data_independent_launch_count(gpu, scene):
    from weasal_amd import _lib
    from weasal_amd.sampler import SphereSampler
    g, sc = scene
    lib = _lib.lib()
    cfg = GoldenCfg()
    cfg.in_radius = 3.0
    growth = {}
    for tag, n in (("sparse", 20000), ("dense", 90000)):
        p, l = sampler_ref.slab_cloud(31, n, 9.0, 1.0, 0.4)
        for S in (4, 8):
            s = SphereSampler(cfg, [(torch.from_numpy(p).to(gpu), torch.from_numpy(l).to(gpu))], seed=5, max_spheres=S,
                              batch_limit=2000 if tag == "sparse" else 500)
            torch.cuda.synchronize()
            before, syncs = lib.ws_launch_count(), s._sync_count
            out = s.sample(capacity_rows=200000)
            growth[(tag, S)] = (lib.ws_launch_count() - before, len(out[3]))
            assert s._sync_count - syncs == 1
    assert growth[("sparse", 4)][0] == growth[("dense", 4)][0] == 1 + 3 * 4
    assert growth[("sparse", 8)][0] == growth[("dense", 8)][0] == 1 + 3 * 8
    assert growth[("sparse", 8)][1] != growth[("dense", 8)][1], "the two tiles were meant to give batches of different sizes"


@pytest.mark.gpu
def test_sampler_feeds_the_prefetcher_the_votes_and_a_training_step(gpu):
    from weasal_amd import config as wcfg, ops, synthetic
    from weasal_amd.architectures import KPFCNN
    from weasal_amd.prefetch import PyramidPrefetcher
    from weasal_amd.sampler import SphereSampler
    from weasal_amd.tester import VoteAccumulator
    from weasal_amd.trainer import make_optimizer, train_step
    wl = synthetic.WORKLOADS["vaihingen"]
    cfg = wcfg.Vaihingen3DPLConfig()
    cfg.in_radius, cfg.in_features_dim, cfg.dropout = wl["radius"], 3, 0.0
    rs = np.random.RandomState(8)
    clouds = []
    for half in (10.0, 8.0):
        raw = (rs.uniform(-1, 1, size=(int(44 * half * half * 4), 3)) * np.array([half, half, 2.0])).astype(np.float32)
        P = torch.from_numpy(raw).to(gpu)
        sub = ops.grid_subsample(P, np.array([P.shape[0]], np.int32), cfg.first_subsampling_dl)[0]
        clouds.append((sub, torch.from_numpy(rs.randint(0, 9, size=sub.shape[0]).astype(np.int32)).to(gpu)))
    s = SphereSampler(cfg, clouds, label_values=np.arange(9), seed=11, max_spheres=16, batch_limit=3 * wl["points"])

    def source():
        for _ in range(3):
            yield s.sample()
    pf = PyramidPrefetcher(cfg, source(), wl["limits"], depth=2, device=gpu, seed=1, workers=1)
    np.random.seed(3)
    torch.manual_seed(3)
    net = KPFCNN(cfg, np.arange(9), []).to(gpu).train()
    opt = make_optimizer(net, cfg)
    votes = VoteAccumulator([c[0].shape[0] for c in clouds], 9, gpu)
    seen = 0
    for batch in pf:
        n0 = batch.points[0].shape[0]
        lens = batch.lengths[0].cpu().numpy()
        assert batch.input_inds.shape == (n0,) and batch.input_inds.dtype == torch.int64 and lens.sum() == n0
        assert batch.cloud_inds.shape == batch.center_inds.shape == (len(lens),) and batch.rots.shape == (len(lens), 3, 3)
        assert batch.scales.shape == (len(lens), 3)
        loss, out = train_step(net, opt, batch, cfg)
        assert out.shape == (n0, 9) and np.isfinite(float(loss.detach()))
        votes.update(out.detach(), batch.points[0], lens, batch.input_inds, batch.cloud_inds)
        i0 = 0
        ci = batch.cloud_inds.cpu().numpy()
        ii = batch.input_inds.cpu().numpy()
        for n, c in zip(lens, ci):                               # every voted row is a member of its sphere's cloud
            idx = ii[i0:i0 + n]
            assert idx.min() >= 0 and idx.max() < clouds[c][0].shape[0] and (np.diff(idx) > 0).all()
            assert (votes.probs[c][torch.from_numpy(idx).to(gpu)].sum(1) > 0).all()
            i0 += n
        seen += 1
    pf.close()
    assert seen == 3
