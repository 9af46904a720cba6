"""GPU: the sphere sampler's colour columns (ws_sampler_set_colors, ws_sampler_batch_items), its random mode
(`random_item`) and the class-balanced centre draw (ws_sampler_class_counts / _select) against golden g18_sampler_items.npz
and tests/sampler_items_ref.py, and the `intensity` field of the cached sub-clouds.  Integers are compared for equality and
floats bit for bit: no tolerance anywhere."""
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import golden

import sampler_items_ref as sir
from test_sampler_cpu import golden_draws, golden_scene
from test_sampler_gpu import as_numpy, assert_same_batch, bits_equal
from test_sampler_gpu import make_sampler as make_g15_sampler
from test_sampler_items_cpu import assert_batch_equals_g18, g18_draws, g18_scene

V3D = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cache_v3d")
DALES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cache")


class Cfg:
    """the configuration golden g18 was made with (make_golden_sampler_items.py)"""
    in_features_dim = 4
    augment_rotation = 'vertical'
    augment_scale_anisotropic = True
    augment_scale_min = 0.9
    augment_scale_max = 1.1
    augment_symmetries = [True, False, False]
    augment_noise = 0.0
    augment_color = 0.7
    batch_num = 4
    epoch_steps = 12
    validation_size = 7
    num_classes = 8
    in_radius = sir.IN_RADIUS


def make_sampler(g, scene, dev, fd=4, colours=True, use_potentials=True, which=(0, 1), **kw):
    from weasal_amd.sampler import SphereSampler
    clouds, pot_points, pots0 = scene
    cfg = Cfg()
    cfg.in_features_dim = fd
    kw.setdefault('max_spheres', int(g['max_spheres']))
    kw.setdefault('seed', 3)
    dev_clouds = []
    for i in which:
        p, l, c = clouds[i]
        entry = (torch.tensor(p).to(dev), torch.tensor(l).to(dev)) + ((torch.tensor(c).to(dev),) if colours else ())
        dev_clouds.append(entry)
    s = SphereSampler(cfg, dev_clouds, label_values=g['label_values'], ignored_labels=tuple(int(v) for v in g['ignored']),
                      batch_limit=int(g['batch_limit']), use_potentials=use_potentials, **kw)
    if use_potentials:
        for j, i in enumerate(which):                          # the HIP grid subsampling equals the CPU oracle's (K2)
            assert bits_equal(s.pot_points[j].cpu().numpy(), pot_points[i])
        s.set_potentials([pots0[i] for i in which])
    return s


@pytest.fixture(scope="module")
def scene():
    g = golden("g18_sampler_items.npz")
    return g, g18_scene(g)


@pytest.mark.gpu
@pytest.mark.parametrize("fd", [4, 2, 1])
def test_four_chained_vaihingen_batches_with_a_colour_column_equal_the_golden(gpu, scene, fd):
    g, sc = scene
    s = make_sampler(g, sc, gpu, fd=fd)
    kept_flags = set()
    for b in range(4):
        d = g18_draws(g, 'b%d' % b)
        got = as_numpy(s.sample(draws=d, capacity_rows=20000))         # roomy: one read per batch
        pots = [p.cpu().numpy() for p in s.potentials]
        assert_batch_equals_g18(g, 'b%d' % b, got, fd, pots)
        assert got['labels'].dtype == np.int64 and got['input_inds'].dtype == np.int64 and got['lengths'].dtype == np.int32
        assert bits_equal(s.last_centres, g['b%d/centres' % b])
        # (min, first arg-min) of every cloud's potentials, as the next batch's picks will read them
        assert np.array_equal([int(np.argmin(p)) for p in pots], g['b%d/argmin_potentials' % b])
        assert np.array_equal([p.min() for p in pots], g['b%d/min_potentials' % b])
        kept = s.last_state[1][:s.last_state[0]['attempts']]
        kept_flags |= {int(d['colour_keep'][k]) for k in np.nonzero(kept[:, 4] >= 0)[0]}
    assert kept_flags == {0, 1} and s.failed == 0 and s._sync_count == 4


@pytest.mark.gpu
def test_a_colourless_sampler_through_the_items_entry_equals_ws_sampler_batch(gpu):
    g = golden("g15_sampler.npz")
    sc = golden_scene(g)
    for tag in ('b0', 'drop'):
        d = golden_draws(g, tag)
        old, new = make_g15_sampler(g, sc, gpu), make_g15_sampler(g, sc, gpu)
        new.through_items = True
        a, b = as_numpy(old.sample(draws=d)), as_numpy(new.sample(draws=d))
        assert_same_batch(a, b)
        for p, q in zip(old.potentials, new.potentials):
            assert bits_equal(p.cpu().numpy(), q.cpu().numpy())
        assert old.last_state[0] == new.last_state[0] and np.array_equal(old.last_state[1], new.last_state[1])
        assert old.last_failed == new.last_failed == (1 if tag == 'drop' else 0)


@pytest.mark.gpu
def test_random_mode_batches_wrap_retry_and_drop(gpu, scene):
    g, sc = scene
    S, limit, lut = int(g['max_spheres']), int(g['batch_limit']), g['lut']
    epoch_inds = g['epoch0/inds']
    s = make_sampler(g, sc, gpu, use_potentials=False)
    assert s.potentials == [] and s.pot_points == []
    s.set_epoch_inds(epoch_inds)
    for tag in ('r0', 'r1', 'r2', 'rdrop'):
        got = as_numpy(s.sample(draws=g18_draws(g, tag), capacity_rows=20000))
        assert_batch_equals_g18(g, tag, got, 4)
        assert int(s.epoch_i.item()) == int(g[tag + '/epoch_i']) and s.last_failed == int(g[tag + '/n_fail'])
    # the lifted slot was dropped, counted, and took its epoch index; the batch went on
    head, slots = s.last_state
    assert s.failed == 1 and slots[1, 4] == -1 and slots[1, 0] < 2 and head['attempts'] == len(got['lengths']) + 1
    assert s._sync_count == 4
    # epoch_i wraps at the end of the list
    n_centres = epoch_inds.shape[1]
    ref = sir.RefItems(sc[0], float(g['in_radius']))
    ref.epoch_inds, ref.epoch_i = epoch_inds, n_centres - 2
    s.epoch_i.fill_(n_centres - 2)
    d = g18_draws(g, 'r0')
    want = ref.batch(d, S, limit, fd=4, lut=lut, random=True)
    got = as_numpy(s.sample(draws=d))
    assert len(want['lengths']) >= 3 and ref.epoch_i == len(want['lengths']) - 2
    assert int(s.epoch_i.item()) == ref.epoch_i
    for k in ('lengths', 'cloud_inds', 'point_inds', 'input_inds', 'labels'):
        assert np.array_equal(got[k], want[k]), k
    for k in ('points', 'features', 'scales', 'rots'):
        assert bits_equal(got[k], want[k]), k
    # a capacity retry resumes the same sphere, epoch_i unchanged by the undone one
    roomy = make_sampler(g, sc, gpu, use_potentials=False)
    roomy.set_epoch_inds(epoch_inds)
    want = as_numpy(roomy.sample(draws=d, capacity_rows=100000))
    assert roomy._sync_count == 1
    # set 'test': the same spheres with zero labels, as in the potential mode
    t = make_sampler(g, sc, gpu, use_potentials=False, set='test')
    t.set_epoch_inds(epoch_inds)
    got = as_numpy(t.sample(draws=d, capacity_rows=100000))
    assert not got['labels'].any() and want['labels'].any()
    for k in ('points', 'features', 'lengths', 'input_inds', 'point_inds', 'cloud_inds'):
        assert bits_equal(got[k], want[k]), k
    for cap in (100, 3000, int(np.sum(want['lengths'])) - 1):           # the first, the second, the last sphere does not fit
        t = make_sampler(g, sc, gpu, use_potentials=False)
        t.set_epoch_inds(epoch_inds)
        got = as_numpy(t.sample(draws=d, capacity_rows=cap))
        assert t._sync_count >= 2, "the small buffer must have been noticed"
        assert_same_batch(got, want)
        assert int(t.epoch_i.item()) == int(roomy.epoch_i.item()) == len(want['lengths']) and t.seq == roomy.seq


@pytest.mark.gpu
def test_random_mode_changes_no_potential(gpu, scene):
    """a sampler built WITH potentials and switched to the list: same batch as golden r0, every potential buffer and the
    potential mode's next pick untouched"""
    g, sc = scene
    s = make_sampler(g, sc, gpu)
    before = [p.cpu().numpy() for p in s.potentials]
    s.use_potentials = False
    s.set_epoch_inds(g['epoch0/inds'])
    got = as_numpy(s.sample(draws=g18_draws(g, 'r0')))
    assert_batch_equals_g18(g, 'r0', got, 4)
    for p, w in zip(s.potentials, before):
        assert bits_equal(p.cpu().numpy(), w)
    s.use_potentials = True
    got = as_numpy(s.sample(draws=g18_draws(g, 'b0')))
    assert_batch_equals_g18(g, 'b0', got, 4, [p.cpu().numpy() for p in s.potentials])


@pytest.mark.gpu
def test_epoch_draw_equals_the_references_iter_and_follows_revealed_labels(gpu, scene):
    from weasal_amd import _lib
    g, sc = scene
    lib = _lib.lib()
    s = make_sampler(g, sc, gpu, use_potentials=False)
    for e in range(2):
        s.rng = np.random.RandomState(int(g['epoch%d/seed' % e]))
        reads = s._epoch_sync_count
        inds = s.draw_epoch_centres(int(g['epoch%d/steps' % e]))
        assert s._epoch_sync_count - reads == 1
        assert inds.dtype == torch.int64 and np.array_equal(inds.cpu().numpy(), g['epoch%d/inds' % e])
        assert np.array_equal(s.last_class_counts, g['class_counts']) and int(s.epoch_i.item()) == 0
        assert s.rng.rand() == float(g['epoch%d/next_rand' % e])
    # a few hundred labels overwritten in the resident buffer: the next draw follows them
    labels = [l.copy() for _, l, _ in sc[0]]
    rs = np.random.RandomState(4)
    for c in range(2):
        ids = rs.choice(len(labels[c]), size=300, replace=False)
        truth = labels[c].copy()
        truth[ids] = rs.randint(0, 9, size=300)
        s.reveal_labels(c, ids, truth)
        labels[c] = truth
    for c in range(2):
        assert np.array_equal(s.sub_labels[c].cpu().numpy(), labels[c])
    s.rng = np.random.RandomState(99)
    inds = s.draw_epoch_centres(12)
    want = sir.epoch_draw(labels, g['label_values'], tuple(g['ignored']), sir.NUM_CLASSES, 48, np.random.RandomState(99))
    assert np.array_equal(inds.cpu().numpy(), want) and not np.array_equal(want, g['epoch0/inds'])
    # launches: the same for the sparse and for the dense cloud
    growth = {}
    for tag, which in (("sparse", (0,)), ("dense", (1,))):
        t = make_sampler(g, sc, gpu, use_potentials=False, which=which)
        torch.cuda.synchronize()
        before = lib.ws_launch_count()
        out = t.draw_epoch_centres(6)
        growth[tag] = lib.ws_launch_count() - before
        lab = sc[0][which[0]][1]
        want = sir.epoch_draw([lab], g['label_values'], tuple(g['ignored']), sir.NUM_CLASSES, 24, np.random.RandomState(3))
        assert np.array_equal(out.cpu().numpy(), want), tag
    assert growth["sparse"] == growth["dense"] > 0


@pytest.mark.gpu
def test_launches_and_reads_per_batch(gpu, scene):
    from weasal_amd import _lib
    g, sc = scene
    lib = _lib.lib()
    for S in (4, 8):
        s = make_sampler(g, sc, gpu, max_spheres=S)
        torch.cuda.synchronize()
        before, syncs = lib.ws_launch_count(), s._sync_count
        s.sample(capacity_rows=200000)
        assert lib.ws_launch_count() - before == 1 + 3 * S and s._sync_count - syncs == 1
    growth = {}
    for tag, which in (("sparse", (0,)), ("dense", (1,))):
        s = make_sampler(g, sc, gpu, use_potentials=False, which=which, max_spheres=8)
        s.rng = np.random.RandomState(5)
        s.draw_epoch_centres(6)
        torch.cuda.synchronize()
        before, syncs = lib.ws_launch_count(), s._sync_count
        out = s.sample(capacity_rows=200000)
        growth[tag] = (lib.ws_launch_count() - before, int(out[0].shape[0]))
        assert s._sync_count - syncs == 1
    assert growth["sparse"][0] == growth["dense"][0] == 1 + 3 * 8          # the formula of DESIGN.md section 10
    assert growth["sparse"][1] != growth["dense"][1], "the two tiles were meant to give batches of different sizes"


@pytest.mark.gpu
def test_refusals(gpu, scene):
    from weasal_amd import _lib
    g, sc = scene
    with pytest.raises(ValueError, match='^Only accepted input dimensions are 1, 2 and 4$'):
        make_sampler(g, sc, gpu, fd=3)
    with pytest.raises(ValueError, match='^Only accepted input dimensions are 1 and 3$'):
        make_sampler(g, sc, gpu, fd=4, colours=False)
    s = make_sampler(g, sc, gpu, fd=4)
    s.config.in_features_dim = 3                                 # the width changed under a live sampler
    with pytest.raises(ValueError, match='^Only accepted input dimensions are 1, 2 and 4$'):
        s.sample(draws=g18_draws(g, 'b0'))
    # the library itself refuses: a width it does not cut, a fourth colour column
    s.config.in_features_dim = 4
    state = torch.empty(s._state_bytes, dtype=torch.uint8, device=gpu)
    out = [torch.empty((10, 3), dtype=torch.float32, device=gpu), torch.empty((10, 3), dtype=torch.float32, device=gpu),
           torch.empty(10, dtype=torch.int64, device=gpu), torch.empty(10, dtype=torch.int64, device=gpu),
           torch.empty(8, dtype=torch.int32, device=gpu), torch.empty((8, 3), dtype=torch.float32, device=gpu),
           torch.empty((8, 3, 3), dtype=torch.float32, device=gpu), torch.empty(8, dtype=torch.int32, device=gpu),
           torch.empty(8, dtype=torch.int32, device=gpu)]
    with pytest.raises(_lib.WeasalHipError, match='status 2: Only accepted input dimensions are 1, 2 and 4'):
        s.handle.batch_items(s._h_draws.data_ptr(), None, 8, 0, 100, 6.5, 0.0, 0, 0, 3, None, False, True, out, 10, state)
    with pytest.raises(_lib.WeasalHipError, match='status 2'):
        s.handle.set_colors(0, torch.zeros((s.sub_points[0].shape[0], 4), dtype=torch.float32, device=gpu))
    # the random mode before any list: refused on the host, nothing is launched
    t = make_sampler(g, sc, gpu, use_potentials=False)
    torch.cuda.synchronize()
    before = _lib.lib().ws_launch_count()
    with pytest.raises(ValueError, match='draw_epoch_centres'):
        t.sample()
    assert _lib.lib().ws_launch_count() == before and t._sync_count == 0
    with pytest.raises(ValueError):
        t.set_potentials([])


@pytest.mark.gpu
@pytest.mark.parametrize("use_potentials", [True, False])
def test_a_sampler_with_colours_feeds_the_prefetcher_and_a_training_step(gpu, use_potentials):
    from weasal_amd import config as wcfg, ops, synthetic
    from weasal_amd.architectures import KPFCNN
    from weasal_amd.prefetch import PyramidPrefetcher
    from weasal_amd.sampler import SphereSampler
    from weasal_amd.trainer import make_optimizer, train_step
    wl = synthetic.WORKLOADS["vaihingen"]
    cfg = wcfg.Vaihingen3DPLConfig()
    cfg.in_radius, cfg.dropout = wl["radius"], 0.0
    assert cfg.in_features_dim == 4
    rs = np.random.RandomState(8)
    clouds = []
    for half in (10.0, 8.0):
        raw = (rs.uniform(-1, 1, size=(int(44 * half * half * 4), 3)) * np.array([half, half, 2.0])).astype(np.float32)
        P = torch.from_numpy(raw).to(gpu)
        sub = ops.grid_subsample(P, np.array([P.shape[0]], np.int32), cfg.first_subsampling_dl)[0]
        lab = torch.from_numpy(rs.randint(0, 9, size=sub.shape[0]).astype(np.int32)).to(gpu)
        col = torch.from_numpy((rs.randint(0, 256, size=(sub.shape[0], 1)) / 255).astype(np.float32)).to(gpu)
        clouds.append((sub, lab, col))
    s = SphereSampler(cfg, clouds, label_values=np.arange(9), seed=11, max_spheres=16, batch_limit=3 * wl["points"],
                      use_potentials=use_potentials)
    if not use_potentials:
        s.draw_epoch_centres(4)

    def source():
        for _ in range(2):
            yield s.sample()
    pf = PyramidPrefetcher(cfg, source(), wl["limits"], depth=2, device=gpu, seed=1, workers=1)
    np.random.seed(3)
    torch.manual_seed(3)
    net = KPFCNN(cfg, np.arange(9), []).to(gpu).train()
    opt = make_optimizer(net, cfg)
    seen = 0
    for batch in pf:
        n0 = batch.points[0].shape[0]
        assert batch.features.shape == (n0, 4) and bool((batch.features[:, 0] == 1).all())
        assert float(batch.features[:, 1].min()) >= 0.0 and float(batch.features[:, 1].max()) <= 1.0
        loss, out = train_step(net, opt, batch, cfg)
        assert out.shape == (n0, 9) and np.isfinite(float(loss.detach()))
        seen += 1
    pf.close()
    assert seen == 2


@pytest.mark.gpu
def test_cache_with_the_intensity_field_is_the_reference_cache(tmp_path, gpu):
    from weasal_amd import cloud_cache
    dl = 0.4
    root = str(tmp_path)
    tile = os.path.join(root, "tile_v.ply")
    shutil.copy(os.path.join(V3D, "tile_v.ply"), tile)
    fixture = os.path.join(V3D, "input_0.400", "tile_v.ply")
    sub_p, sub_l, sub_c, built = cloud_cache.load_subsampled_cloud(root, "tile_v", tile, dl, gpu, color_field='intensity')
    assert built and sub_c.dtype == torch.float32 and sub_c.shape == (sub_p.shape[0], 1) and sub_l.dtype == torch.int32
    mine = os.path.join(cloud_cache.cache_dir(root, dl), "tile_v.ply")
    assert open(mine, "rb").read() == open(fixture, "rb").read()
    pts, lab, col = cloud_cache.read_sub_cloud(fixture, 'intensity')
    assert bits_equal(sub_c.cpu().numpy(), col) and bits_equal(sub_p.cpu().numpy(), pts) and np.array_equal(sub_l.cpu().numpy(), lab)
    p2, l2, c2, built2 = cloud_cache.load_subsampled_cloud(root, "tile_v", tile, dl, gpu, color_field='intensity')
    assert not built2 and bits_equal(c2.cpu().numpy(), col) and bits_equal(p2.cpu().numpy(), pts)
    # the default call writes what it writes today
    root2 = str(tmp_path / "dales")
    os.makedirs(root2)
    tile_a = os.path.join(root2, "tile_a.ply")
    shutil.copy(os.path.join(DALES, "tile_a.ply"), tile_a)
    out = cloud_cache.load_subsampled_cloud(root2, "tile_a", tile_a, dl, gpu)
    assert len(out) == 3 and out[2] is True
    assert open(os.path.join(cloud_cache.cache_dir(root2, dl), "tile_a.ply"), "rb").read() == \
        open(os.path.join(DALES, "input_0.400", "tile_a.ply"), "rb").read()
