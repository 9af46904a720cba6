"""CPU (no GPU needed): the sphere sampler's colour columns, `random_item` and the class-balanced centre draw --
tests/sampler_items_ref.py against golden g18_sampler_items.npz (whose generator holds it to the reference's own code), and
the host halves of weasal_amd.sampler (draw_slots, draw_epoch_positions) against both.  Equal, not close, everywhere."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from conftest import golden

import sampler_items_ref as sir

DRAW_KEYS = ('noise', 'R', 'scale', 'colour_keep')


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


_SCENE = {}


def g18_scene(g):
    """the clouds of the golden, rebuilt from their seeds once and checked against the stored digests
    -> (clouds [(points, labels, colours)], pot_points, pots0); nobody writes into them"""
    if not _SCENE:
        assert np.array_equal(g['clouds'], np.array(sir.CLOUDS, np.float64))
        clouds = sir.scene()
        pot_points = []
        for i, (p, l, c) in enumerate(clouds):
            assert len(p) == int(g['sub_n_%d' % i]) and np.array_equal(digest(p), g['sub_sha_%d' % i])
            assert np.array_equal(digest(l), g['labels_sha_%d' % i]) and np.array_equal(digest(c), g['colors_sha_%d' % i])
            pot_points.append(sir.potential_points(p, float(g['in_radius'])))
            assert np.array_equal(digest(pot_points[i]), g['pot_points_sha_%d' % i])
            for a in (p, l, c, pot_points[i]):
                a.setflags(write=False)
        _SCENE['v'] = (clouds, pot_points, [g['pots0_%d' % i] for i in range(len(clouds))])
    return _SCENE['v']


def g18_draws(g, tag):
    return {k: g['%s/draws_%s' % (tag, k)] for k in DRAW_KEYS}


def assert_batch_equals_g18(g, tag, res, fd=4, potentials=None):
    """res: dict of numpy arrays (the nine outputs, features of width fd); potentials: float64 arrays after the batch"""
    for key in ('lengths', 'cloud_inds', 'point_inds'):
        assert np.array_equal(np.asarray(res[key]).astype(np.int64), g['%s/%s' % (tag, key)].astype(np.int64)), (tag, key)
    assert np.array_equal(digest(np.asarray(res['input_inds']).astype(np.int64)), g[tag + '/input_inds_sha']), tag
    assert np.array_equal(np.asarray(res['labels']).astype(np.int64), g[tag + '/labels'].astype(np.int64)), tag
    for key in ('scales', 'rots'):
        assert np.array_equal(np.asarray(res[key], np.float32).view(np.int32), g['%s/%s' % (tag, key)].view(np.int32)), (tag, key)
    assert res['points'].dtype == np.float32 and res['features'].dtype == np.float32 and res['features'].shape[1] == fd
    assert np.array_equal(digest(res['points']), g[tag + '/points_sha']), tag + ": points differ in some bit"
    assert np.array_equal(digest(res['features']), g['%s/features%d_sha' % (tag, fd)]), tag + ": features differ in some bit"
    if tag + '/points' in g.files:                              # the first batch is stored in full
        assert np.array_equal(res['points'].view(np.int32), g[tag + '/points'].view(np.int32))
        assert np.array_equal(np.asarray(res['input_inds']).astype(np.int64), g[tag + '/input_inds'].astype(np.int64))
        full = np.hstack((np.ones((len(res['points']), 1), np.float32), g[tag + '/features_1_2'], g[tag + '/points'][:, 2:]))
        assert np.array_equal(res['features'].view(np.int32), np.ascontiguousarray(full[:, :fd]).view(np.int32))
    if potentials is not None:
        for i, p in enumerate(potentials):
            assert p.dtype == np.float64 and np.array_equal(digest(p), g['%s/pot_sha_%d' % (tag, i)]), (tag, "potentials of cloud", i)


def test_the_restatement_reproduces_the_golden_bit_for_bit():
    g = golden("g18_sampler_items.npz")
    clouds, pot_points, pots0 = g18_scene(g)
    S, limit, lut = int(g['max_spheres']), int(g['batch_limit']), g['lut']
    refs = {fd: sir.RefItems(clouds, float(g['in_radius']), pot_points, pots0) for fd in (4, 2, 1)}
    kept_flags = set()
    for b in range(4):
        d = g18_draws(g, 'b%d' % b)
        for fd, ref in refs.items():
            res = ref.batch(d, S, limit, fd=fd, lut=lut)
            assert_batch_equals_g18(g, 'b%d' % b, res, fd, ref.potentials)
            assert np.array_equal(ref.min_potentials, g['b%d/min_potentials' % b])
            assert np.array_equal(ref.argmin_potentials, g['b%d/argmin_potentials' % b])
            assert np.array_equal(res['centres'], g['b%d/centres' % b]) and res['n_fail'] == 0
            assert np.sum(res['lengths'][:-1]) <= limit < np.sum(res['lengths'])
        kept_flags |= {int(d['colour_keep'][k]) for k in res['slots']}
    assert kept_flags == {0, 1}
    rnd = sir.RefItems(clouds, float(g['in_radius']))
    rnd.epoch_inds = g['epoch0/inds']
    for tag in ('r0', 'r1', 'r2', 'rdrop'):
        res = rnd.batch(g18_draws(g, tag), S, limit, fd=4, lut=lut, random=True)
        assert_batch_equals_g18(g, tag, res, 4)
        assert rnd.epoch_i == int(g[tag + '/epoch_i']) and res['n_fail'] == int(g[tag + '/n_fail'])
    assert int(g['rdrop/n_fail']) == 1 and rnd.failed == 1
    # the colour column of the first batch: the tile's value where the slot kept it, +0.0 where it dropped it
    ref = sir.RefItems(clouds, float(g['in_radius']), pot_points, pots0)
    d = g18_draws(g, 'b0')
    res = ref.batch(d, S, limit, fd=2, lut=lut)
    i0 = 0
    for kept, k in enumerate(res['slots']):
        n, ci = int(res['lengths'][kept]), int(res['cloud_inds'][kept])
        want = clouds[ci][2][res['input_inds'][i0:i0 + n], 0] if d['colour_keep'][k] else np.zeros(n, np.float32)
        assert np.array_equal(res['features'][i0:i0 + n, 1].view(np.int32), want.view(np.int32))
        i0 += n
    with pytest.raises(ValueError, match='Only accepted input dimensions are 1, 2 and 4'):
        ref.batch(d, S, limit, fd=3, lut=lut)


def test_the_position_draw_needs_only_the_counts_and_leaves_the_stream_where_the_reference_does():
    from weasal_amd.sampler import draw_epoch_positions
    g = golden("g18_sampler_items.npz")
    clouds, _, _ = g18_scene(g)
    labels = [l for _, l, _ in clouds]
    values = [v for v in g['label_values'] if v not in g['ignored']]
    counts = np.array([[int(np.sum(l == v)) for v in values] for l in labels], np.int64)
    assert np.array_equal(counts, g['class_counts'])
    for e in range(2):
        n_centres = int(g['epoch%d/steps' % e]) * int(g['epoch%d/batch_num' % e])
        rs = np.random.RandomState(int(g['epoch%d/seed' % e]))
        tri = draw_epoch_positions(counts, n_centres, rs)
        assert rs.rand() == float(g['epoch%d/next_rand' % e])
        assert tri.dtype == np.int64 and np.array_equal(tri, g['epoch%d/triples' % e])
        inds = np.array([tri[:, 0], [np.where(labels[c] == values[k])[0][p] for c, k, p in tri]], np.int64)
        assert np.array_equal(inds, g['epoch%d/inds' % e])
        rs = np.random.RandomState(int(g['epoch%d/seed' % e]))
        ours = sir.epoch_draw(labels, g['label_values'], tuple(g['ignored']), sir.NUM_CLASSES, n_centres, rs)
        assert np.array_equal(ours, g['epoch%d/inds' % e]) and rs.rand() == float(g['epoch%d/next_rand' % e])
    assert g['epoch0/inds'].shape[1] < 48 and g['epoch1/inds'].shape[1] == 28          # nothing to cut / the cut bites


class _Cfg:
    augment_rotation = 'vertical'
    augment_scale_anisotropic = True
    augment_scale_min = 0.9
    augment_scale_max = 1.1
    augment_symmetries = [True, False, False]
    augment_color = 0.7
    in_radius = 6.5


def _host_sampler(ncol, seed, set='training'):
    """a SphereSampler with nothing but what draw() reads (its constructor needs a device)"""
    from weasal_amd.sampler import SphereSampler
    s = SphereSampler.__new__(SphereSampler)
    s.config, s.rng, s.set, s.max_spheres, s.ncol = _Cfg(), np.random.RandomState(seed), set, 8, ncol
    return s


def test_a_colourless_draw_consumes_exactly_what_it_consumed_before():
    from weasal_amd.sampler import DRAW_DTYPE, draw_augmentation
    for set in ('training', 'ERF'):
        s = _host_sampler(0, 77, set)
        twin = np.random.RandomState(77)
        d = s.draw()
        assert isinstance(d, np.ndarray) and d.dtype == DRAW_DTYPE and d.shape == (8,)
        for k in range(8):
            noise = twin.normal(scale=6.5 / 10, size=(1, 3))[0] if set != 'ERF' else np.zeros(3)
            R, scale = draw_augmentation(s.config, twin)
            assert np.array_equal(d['noise'][k], noise) and np.array_equal(d['R'][k], R) and np.array_equal(d['scale'][k], scale)
        assert s.rng.rand() == twin.rand()


def test_with_colours_draw_takes_one_more_rand_per_slot_after_the_augmentation_draws():
    from weasal_amd.sampler import draw_augmentation
    g = golden("g18_sampler_items.npz")
    s = _host_sampler(1, 78)
    twin = np.random.RandomState(78)
    d = s.draw()
    assert sorted(d) == sorted(DRAW_KEYS) and d['colour_keep'].shape == (8,)
    for k in range(8):
        noise = twin.normal(scale=6.5 / 10, size=(1, 3))[0]
        R, scale = draw_augmentation(s.config, twin)
        keep = 0 if twin.rand() > s.config.augment_color else 1
        assert np.array_equal(d['noise'][k], noise) and np.array_equal(d['R'][k], R) and np.array_equal(d['scale'][k], scale)
        assert d['colour_keep'][k] == keep
    assert s.rng.rand() == twin.rand() and set(d['colour_keep'].tolist()) == {0, 1}
    # the golden's draws were made the same way, one seed per slot
    from weasal_amd.sampler import draw_slots
    for k in range(8):
        dk, kk = draw_slots(s.config, np.random.RandomState(18000 + k), 1, colours=True)
        assert np.array_equal(dk['noise'][0], g['b0/draws_noise'][k]) and np.array_equal(dk['R'][0], g['b0/draws_R'][k])
        assert np.array_equal(dk['scale'][0], g['b0/draws_scale'][k]) and kk[0] == g['b0/draws_colour_keep'][k]


def test_cached_sub_cloud_with_intensity_reads_and_rewrites_identically(tmp_path):
    """the reference-written Vaihingen3D-style cache file (x y z intensity class): read with its colours, written back as
    the same bytes; the oracle's subsampling with features + `/ 255` in float32 + our writer give that file too; a
    two-field caller reads the same file as before"""
    import os
    from oracle import geom
    from weasal_amd import cloud_cache
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cache_v3d")
    ref_file = os.path.join(cloud_cache.cache_dir(here, 0.4), "tile_v.ply")
    pts, lab, col = cloud_cache.read_sub_cloud(ref_file, 'intensity')
    assert pts.dtype == np.float32 and col.dtype == np.float32 and col.shape == (len(pts), 1) and lab.dtype == np.int32
    assert 0.0 <= col.min() and col.max() <= 1.0
    out = str(tmp_path / "again.ply")
    assert cloud_cache.write_sub_cloud(out, pts, lab, col, 'intensity')
    assert open(out, "rb").read() == open(ref_file, "rb").read()
    points, colors, labels = cloud_cache.read_tile_colors(os.path.join(here, "tile_v.ply"), 'intensity')
    sub_p, sub_f, sub_l = geom.subsample(points, features=colors, classes=labels.astype(np.int32), sampleDl=0.4)
    out2 = str(tmp_path / "sub.ply")
    assert cloud_cache.write_sub_cloud(out2, sub_p, np.squeeze(sub_l), (sub_f / 255).astype(np.float32), 'intensity')
    assert open(out2, "rb").read() == open(ref_file, "rb").read()
    p2, l2 = cloud_cache.read_sub_cloud(ref_file)
    assert np.array_equal(p2, pts) and np.array_equal(l2, lab)


def test_the_new_entries_are_exported_mirrored_and_validate_without_a_device():
    from weasal_amd import _lib, ops
    from weasal_amd.sampler import check_dims
    lib = _lib.lib()
    for name in ("ws_sampler_set_colors", "ws_sampler_batch_items", "ws_sampler_items_bytes", "ws_sampler_class_counts",
                 "ws_sampler_class_select"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert C.sizeof(ops.SamplerItems) == lib.ws_sampler_items_bytes()
    assert lib.ws_sampler_state_bytes() == 8 * (8 + 64 * 8) and lib.ws_sampler_draw_bytes() == 72       # unchanged
    null = C.c_void_p(None)
    assert lib.ws_sampler_batch_items(null, null) == 1 and lib.ws_sampler_set_colors(null, 0, null, 1, null) == 1
    assert lib.ws_sampler_class_counts(null, null, 8, null, null) == 1
    assert lib.ws_sampler_class_select(null, null, 8, null, 4, null, null) == 1
    for fd, ncol in ((1, 0), (3, 0), (1, 1), (2, 1), (4, 1), (4, 3), (6, 3)):
        check_dims(fd, ncol)
    with pytest.raises(ValueError, match='^Only accepted input dimensions are 1 and 3$'):
        check_dims(4, 0)
    with pytest.raises(ValueError, match='^Only accepted input dimensions are 1, 2 and 4$'):
        check_dims(3, 1)
