"""CPU (no GPU needed): the sphere sampler's reference restatement against its golden, the host-side draw logic against
the reference's augmentation_transform, and the ABI of the new library entries.

g15_sampler.npz (tests/golden/make_golden_sampler.py) holds six chained batches over two slab clouds, a batch with a
dropped sphere, and the (R, scale) the reference's own augmentation_transform drew for every augmentation mode.  Large
arrays are stored as SHA-256 digests: equal digests are equal bits."""
import hashlib

import numpy as np

from conftest import golden

import sampler_ref

DRAW_DTYPE = np.dtype([('noise', np.float64, (3,)), ('R', np.float32, (3, 3)), ('scale', np.float32, (3,))])


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def golden_scene(g):
    """the clouds of the golden, regenerated from their seeds and checked against the stored digests"""
    lv = g['label_values']
    clouds, pot_points, pots0 = [], [], []
    for i, (seed, n, half, zhalf) in enumerate(g['clouds']):
        p, l = sampler_ref.slab_cloud(int(seed), int(n), float(half), float(zhalf), float(g['dl']))
        l = lv[l].astype(np.int32)
        assert len(p) == int(g['sub_n_%d' % i]) and np.array_equal(digest(p), g['sub_sha_%d' % i])
        assert np.array_equal(digest(l), g['labels_sha_%d' % i])
        pp = sampler_ref.potential_points(p, float(g['in_radius']))
        assert np.array_equal(digest(pp), g['pot_points_sha_%d' % i])
        clouds.append((p, l)); pot_points.append(pp); pots0.append(g['pots0_%d' % i])
    return clouds, pot_points, pots0


def golden_draws(g, tag):
    d = np.zeros(int(g['max_spheres']), DRAW_DTYPE)
    d['noise'], d['R'], d['scale'] = g[tag + '/draws_noise'], g[tag + '/draws_R'], g[tag + '/draws_scale']
    return d


def assert_batch_equals_golden(g, tag, res, potentials):
    """res: dict of numpy arrays (the nine outputs); potentials: list of float64 arrays after the batch"""
    for key in ('lengths', 'cloud_inds', 'point_inds'):
        assert np.array_equal(np.asarray(res[key]).astype(np.int64), g['%s/%s' % (tag, key)].astype(np.int64)), (tag, key)
    assert np.array_equal(np.asarray(res['input_inds']).astype(np.int64), g[tag + '/input_inds'].astype(np.int64)), tag
    assert np.array_equal(np.asarray(res['labels']).astype(np.int64), g[tag + '/labels'].astype(np.int64)), tag
    for key in ('scales', 'rots'):
        assert np.array_equal(np.asarray(res[key], np.float32).view(np.int32), g['%s/%s' % (tag, key)].view(np.int32)), (tag, key)
    assert res['points'].dtype == np.float32 and res['features'].dtype == np.float32
    assert np.array_equal(digest(res['points']), g[tag + '/points_sha']), tag + ": points differ in some bit"
    assert np.array_equal(digest(res['features']), g[tag + '/features_sha']), tag + ": features differ in some bit"
    for i, p in enumerate(potentials):
        assert p.dtype == np.float64 and np.array_equal(digest(p), g['%s/pot_sha_%d' % (tag, i)]), (tag, "potentials of cloud", i)


def test_sampler_ref_reproduces_the_golden_bit_for_bit():
    g = golden("g15_sampler.npz")
    clouds, pot_points, pots0 = golden_scene(g)
    S, limit, lut = int(g['max_spheres']), int(g['batch_limit']), g['lut']
    ref = sampler_ref.RefSampler(clouds, pot_points, pots0, float(g['in_radius']))
    for b in range(6):
        res = ref.batch(golden_draws(g, 'b%d' % b), S, limit, fd=3, lut=lut)
        assert_batch_equals_golden(g, 'b%d' % b, res, ref.potentials)
        assert np.array_equal(ref.min_potentials, g['b%d/min_potentials' % b])
        assert np.array_equal(ref.argmin_potentials, g['b%d/argmin_potentials' % b])
        assert np.array_equal(res['centres'], g['b%d/centres' % b]) and res['n_fail'] == 0
        assert np.sum(res['lengths'][:-1]) <= limit < np.sum(res['lengths'])
        if b == 0:
            assert np.array_equal(res['points'].view(np.int32), g['b0/points'].view(np.int32))
            assert np.array_equal(res['features'].view(np.int32), g['b0/features'].view(np.int32))
    assert len({int(c) for b in range(6) for c in g['b%d/cloud_inds' % b]}) == 2          # the clouds alternate
    for i, p in enumerate(ref.potentials):
        assert np.array_equal(p, g['final_pot_%d' % i])
    ref2 = sampler_ref.RefSampler(clouds, pot_points, pots0, float(g['in_radius']))
    res = ref2.batch(golden_draws(g, 'drop'), S, limit, fd=3, lut=lut)
    assert res['n_fail'] == 1 and int(g['drop/n_fail']) == 1 and res['slots'][0] == 1
    assert_batch_equals_golden(g, 'drop', res, ref2.potentials)


def test_host_draws_equal_the_references_augmentation_transform():
    """sampler.draw_augmentation consumes a RandomState as datasets/common.py:260-302 consumes np.random: same R, same
    scale for 'vertical' / 'all' / 'none', isotropic or not, with and without symmetries"""
    from weasal_amd.sampler import draw_augmentation
    g = golden("g15_sampler.npz")

    class Cfg:
        augment_scale_min = 0.9
        augment_scale_max = 1.1
        in_radius = float(g['in_radius'])
    for m, rot in enumerate(g['mode_rot']):
        cfg = Cfg()
        cfg.augment_rotation = str(rot)
        cfg.augment_scale_anisotropic = bool(g['mode%d/aniso' % m])
        cfg.augment_symmetries = [bool(v) for v in g['mode%d/sym' % m]]
        for j in range(4):
            rng = np.random.RandomState(17000 + 10 * m + j)
            noise = rng.normal(scale=cfg.in_radius / 10, size=(1, 3))[0]
            R, scale = draw_augmentation(cfg, rng)
            assert np.array_equal(noise, g['mode%d/noise' % m][j])
            assert R.dtype == np.float32 and np.array_equal(R.view(np.int32), g['mode%d/R' % m][j].view(np.int32)), (rot, j)
            assert scale.dtype == np.float32 and scale.shape == (3,)
            assert np.array_equal(scale.view(np.int32), g['mode%d/scale' % m][j].view(np.int32)), (rot, j)
        if str(rot) == 'none':
            assert np.array_equal(g['mode%d/R' % m][0], np.eye(3, dtype=np.float32))
    # the batches of the golden were drawn the same way (seed per slot)
    cfg = Cfg()
    cfg.augment_rotation, cfg.augment_scale_anisotropic, cfg.augment_symmetries = 'vertical', True, [True, False, False]
    for k, seed in enumerate(g['b0/seeds']):
        rng = np.random.RandomState(int(seed))
        noise = rng.normal(scale=cfg.in_radius / 10, size=(1, 3))[0]
        R, scale = draw_augmentation(cfg, rng)
        assert np.array_equal(noise, g['b0/draws_noise'][k]) and np.array_equal(R, g['b0/draws_R'][k])
        assert np.array_equal(scale, g['b0/draws_scale'][k])


def test_label_lut_is_label_to_idx():
    from weasal_amd.sampler import label_lut
    lut = label_lut([0, 1, 2, 3, 5, 6, 7, 8, 10])
    assert lut.dtype == np.int32 and lut.tolist() == [0, 1, 2, 3, -1, 4, 5, 6, 7, -1, 10]     # common.py:249-250: 10 stays 10
    assert label_lut([2, 0, 7]).tolist() == [0, -1, 1, -1, -1, -1, -1, 2]


def test_library_exports_the_sampler_entries():
    import ctypes as C
    from weasal_amd import _lib
    lib = _lib.lib()
    for name in ("ws_sampler_create", "ws_sampler_destroy", "ws_sampler_add_cloud", "ws_sampler_state_bytes",
                 "ws_sampler_draw_bytes", "ws_sampler_batch"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.ws_sampler_state_bytes() == 8 * (8 + 64 * 8)
    assert lib.ws_sampler_draw_bytes() == DRAW_DTYPE.itemsize == 72
    null = C.c_void_p(None)
    assert lib.ws_sampler_batch(null, null, 8, 0, 100, 1.0, 0.0, 0, 0, 3, null, 0, 0, 1, null, null, null, null, null, null,
                                null, null, null, 10, null, null) == 1                           # validation needs no device
    assert lib.ws_sampler_add_cloud(null, null, null, 4, null, null, 4, null) == 1
