"""Generates tests/golden/g18_sampler_items.npz (run once in the build container; the reference cannot travel): the sphere
sampler with a colour column (four chained Vaihingen potential batches at in_features_dim 4, 2 and 1), `random_item`
batches and the class-balanced centre draw, over the two slab clouds of tests/sampler_items_ref.py (about 3 000 and about
70 000 sub-points, labels planted so that the draw takes every branch).

The bodies are tests/sampler_items_ref.py.  Held to the reference's OWN code here, at generation time, under the import aids
of make_golden.py and the `mayavi_visu` stub of make_golden_anchors.py:
  (r1) datasets/Vaihingen3D_PseudoLabel.py `Vaihingen3DPLSampler.__iter__` on a stub dataset (`__new__`; use_potentials False,
       epoch_i, epoch_inds, config, num_clouds, input_labels, label_values, ignored_labels) gives the epoch_inds of
       sampler_items_ref.epoch_draw AND of weasal_amd.sampler.draw_epoch_positions fed with the counts alone, for both
       epoch sizes, and all three leave the stream at the same place (next rand() equal); the two identities the position
       draw rests on are asserted on their own: choice(arr, k, replace=False) == arr[choice(len(arr), k, replace=False)],
       np.unique(choice(arr, k)) == arr[np.unique(choice(len(arr), k))] for an ascending arr;
  (r2) the reference's own `potential_item` and `random_item` on a stub whose `segmentation_inputs` hands back its four
       arguments, ONE sphere per call (batch_limit 0) over twelve consecutive spheres with the potentials and epoch_i chained:
       the reference adds the centre noise into its KD-tree's data (`center_point` is a view), so the moved point is put back
       after every call -- the documented difference.  The host draws are replayed from the same np.random seed with
       weasal_amd.sampler.draw_slots' order (centre normal, rotation, scales, symmetries, the n x 3 per-point normals the
       reference draws even at augment_noise 0, then the colour rand()).  Rows are sorted by input index first (the
       KD-tree returns its traversal order); points, the four feature columns, labels, input_inds, lengths, scales, rots,
       cloud_inds, point_inds and the potentials are then equal bit for bit;
  (a) brute-force float64 membership equals the tree's for every sphere; (b) no point within a relative 1e-9 of r^2.
augment_noise is 0 (the per-point noise is the device generator's).  Large arrays are stored as SHA-256 digests next to the
first batch in full.  Usage: python tests/golden/make_golden_sampler_items.py"""
import hashlib
import os
import sys
import threading
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg          # noqa: E402,F401  (import aids; puts the reference on sys.path)
import numpy as np                # noqa: E402
import torch                      # noqa: E402
from sklearn.neighbors import KDTree  # noqa: E402

stub = types.ModuleType("utils.mayavi_visu")
stub.KDTree = KDTree
sys.modules["utils.mayavi_visu"] = stub
from datasets.Vaihingen3D_PseudoLabel import Vaihingen3DPLDataset, Vaihingen3DPLSampler  # noqa: E402
import sampler_items_ref as sir   # noqa: E402
from weasal_amd.sampler import DRAW_DTYPE, draw_augmentation, draw_epoch_positions, draw_slots, label_lut  # noqa: E402

NB = 4
EPOCHS = ((12, 4), (7, 4))        # (steps, batch_num): 48 centres at pick_n 3 (nothing cut), 28 at pick_n 2 (the cut bites)


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


class Cfg:
    augment_rotation = 'vertical'
    augment_scale_anisotropic = True
    augment_scale_min = 0.9
    augment_scale_max = 1.1
    augment_symmetries = [True, False, False]
    augment_noise = 0.0
    augment_color = 0.7
    in_radius = sir.IN_RADIUS
    in_features_dim = 4
    batch_num = 4
    num_classes = sir.NUM_CLASSES
    epoch_steps = 12
    validation_size = 7


def slot_draws(cfg, seeds):
    """per slot: np.random.seed(seed), then the draws of one sphere in weasal_amd.sampler.draw_slots' order"""
    d = np.zeros(len(seeds), DRAW_DTYPE)
    keep = np.zeros(len(seeds), np.int32)
    for k, s in enumerate(seeds):
        dk, kk = draw_slots(cfg, np.random.RandomState(int(s)), 1, colours=True)
        d[k], keep[k] = dk[0], kk[0]
    return {'noise': d['noise'], 'R': d['R'], 'scale': d['scale'], 'colour_keep': keep}


def check_membership(clouds, res):
    r2 = sir.IN_RADIUS * sir.IN_RADIUS
    i0, closest = 0, np.inf
    for kept in range(len(res['lengths'])):
        c, ci, n = res['centres'][kept], int(res['cloud_inds'][kept]), int(res['lengths'][kept])
        dd = clouds[ci][0].astype(np.float64) - c
        rd = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
        assert np.array_equal(np.nonzero(rd <= r2)[0], res['input_inds'][i0:i0 + n]), "(a) brute force differs from the tree"
        closest = min(closest, np.abs(rd - r2).min() / r2)
        assert not (res['points'][i0:i0 + n] == 0).any(), "a zero coordinate"
        i0 += n
    assert closest > 1e-9, "(b) a point within 1e-9 of the radius"
    return closest


def store(out, tag, res, ref=None, full=False):
    for key in ('lengths', 'cloud_inds', 'point_inds', 'scales', 'rots', 'centres', 'slots'):
        out['%s/%s' % (tag, key)] = res[key]
    out[tag + '/n_fail'] = np.int64(res['n_fail'])
    out[tag + '/labels'] = res['labels'].astype(np.int8)
    out[tag + '/input_inds_sha'] = digest(res['input_inds'].astype(np.int64))
    out[tag + '/points_sha'] = digest(res['points'])
    for fd in (4, 2, 1):
        out['%s/features%d_sha' % (tag, fd)] = digest(np.ascontiguousarray(res['features'][:, :fd]))
    if full:
        # in full: the points and feature columns 1, 2; column 0 is all ones and column 3 is the points' z (asserted)
        assert (res['features'][:, 0] == 1).all() and np.array_equal(res['features'][:, 3].view(np.int32), res['points'][:, 2].view(np.int32))
        out[tag + '/points'], out[tag + '/features_1_2'] = res['points'], np.ascontiguousarray(res['features'][:, 1:3])
        out[tag + '/input_inds'] = res['input_inds'].astype(np.int32)
    if ref is not None:
        for i, p in enumerate(ref.potentials):
            out['%s/pot_sha_%d' % (tag, i)] = digest(p)
        out[tag + '/min_potentials'] = ref.min_potentials.copy()
        out[tag + '/argmin_potentials'] = ref.argmin_potentials.copy()


# ---- the reference's own code on stubs -------------------------------------------------------------------------------

def ref_dataset(cfg, clouds, lut, pot_points=None, pots0=None):
    ds = Vaihingen3DPLDataset.__new__(Vaihingen3DPLDataset)
    ds.config, ds.set, ds.batch_limit = cfg, 'training', 0
    ds.worker_lock = threading.Lock()
    ds.input_trees = [KDTree(p, leaf_size=10) for p, _, _ in clouds]
    ds.input_labels = [l for _, l, _ in clouds]
    ds.input_colors = [c for _, _, c in clouds]
    ds.label_to_idx = {int(v): int(lut[v]) for v in sir.LABEL_VALUES}
    ds.segmentation_inputs = lambda p, f, l, s: [p, f, l, s]
    if pot_points is not None:
        ds.pot_trees = [KDTree(p, leaf_size=10) for p in pot_points]
        ds.potentials = [torch.from_numpy(p.copy()) for p in pots0]
        ds.argmin_potentials = torch.tensor([int(torch.argmin(p)) for p in ds.potentials], dtype=torch.int64)
        ds.min_potentials = torch.tensor([float(p[i]) for p, i in zip(ds.potentials, ds.argmin_potentials)], dtype=torch.float64)
    return ds


def replay_one(cfg, seed, n):
    """the draws the reference made for the one sphere of a call seeded with `seed` that kept n points"""
    rs = np.random.RandomState(int(seed))
    d = np.zeros(1, DRAW_DTYPE)
    d['noise'][0] = rs.normal(scale=cfg.in_radius / 10, size=(1, 3))[0]
    d['R'][0], d['scale'][0] = draw_augmentation(cfg, rs)
    rs.randn(n, 3)
    keep = np.array([0 if rs.rand() > cfg.augment_color else 1], np.int32)
    return {'noise': d['noise'], 'R': d['R'], 'scale': d['scale'], 'colour_keep': keep}, rs


def pin_items(cfg, clouds, lut, pot_points, pots0, epoch_inds):
    keeps = set()
    for random in (False, True):
        ds = ref_dataset(cfg, clouds, lut, pot_points, pots0)
        ours = sir.RefItems(clouds, sir.IN_RADIUS, pot_points, pots0)
        if random:
            ds.epoch_inds, ds.epoch_i = torch.from_numpy(epoch_inds.copy()), 0
            ours.epoch_inds, ours.epoch_i = epoch_inds, 0
        for j in range(12):
            trees = ds.input_trees if random else ds.pot_trees
            before = [np.array(t.data, copy=True) for t in trees]
            seed = 18500 + 100 * int(random) + j
            if not random:                                    # every call starts from the restatement's potentials
                ds.potentials = [torch.from_numpy(p.copy()) for p in ours.potentials]
                ds.min_potentials = torch.from_numpy(ours.min_potentials.copy())
                ds.argmin_potentials = torch.from_numpy(ours.argmin_potentials.copy())
                pots_before = [p.copy() for p in ours.potentials]
            np.random.seed(seed)
            got = ds.random_item(j) if random else ds.potential_item(j)
            after_rand = np.random.rand()
            for t, b in zip(trees, before):                   # put the drifted centre back (the documented difference)
                np.array(t.data, copy=False)[...] = b
            pts, feats, labels, lengths, scales, rots, cloud_inds, point_inds, input_inds = got
            assert len(lengths) == 1
            d, rs = replay_one(cfg, seed, int(lengths[0]))
            assert rs.rand() == after_rand, "the replay left the stream elsewhere"
            keeps.add(int(d['colour_keep'][0]))
            want = ours.batch(d, 1, 0, fd=4, lut=lut, random=random)
            order = np.argsort(input_inds, kind='stable')
            assert np.array_equal(input_inds[order], want['input_inds']) and np.array_equal(lengths, want['lengths'])
            rows = np.ones(len(order), bool)
            if random:                # the reference moved the centre's own point onto the centre: that row is (0, 0, 0) there
                own = want['input_inds'] == int(point_inds[0])
                assert own.sum() == 1 and not pts[order][own].any()
                rows = ~own
                assert np.array_equal(feats[order][own][:, :2].view(np.int32), want['features'][own][:, :2].view(np.int32))
            assert pts.dtype == np.float32 and np.array_equal(pts[order][rows].view(np.int32), want['points'][rows].view(np.int32))
            assert feats.dtype == np.float32 and feats.shape[1] == 4
            assert np.array_equal(feats[order][rows].view(np.int32), want['features'][rows].view(np.int32))
            assert np.array_equal(np.asarray(labels)[order].astype(np.int64), want['labels'])
            assert np.array_equal(scales.view(np.int32), want['scales'].view(np.int32)) and np.array_equal(rots, want['rots'])
            assert np.array_equal(cloud_inds, want['cloud_inds']) and np.array_equal(point_inds, want['point_inds'])
            if random:
                assert int(ds.epoch_i) == ours.epoch_i
            else:
                # the reference's centre IS its potential point after the noise went in: distance 0, Tukey weight 1 there
                ci, pi = int(cloud_inds[0]), int(point_inds[0])
                for i, (a, b) in enumerate(zip(ds.potentials, ours.potentials)):
                    same = np.ones(len(b), bool)
                    if i == ci:
                        same[pi] = False
                        assert a.numpy()[pi] == pots_before[i][pi] + 1.0
                    assert np.array_equal(a.numpy()[same], b[same])
    assert keeps == {0, 1}
    print("(r2) twelve spheres of the reference's potential_item and twelve of its random_item equal the restatement")


def pin_epoch_draw(cfg, labels, out):
    arr = np.sort(np.random.RandomState(5).choice(100000, size=700, replace=False))
    a, b = np.random.RandomState(6), np.random.RandomState(6)
    assert np.array_equal(a.choice(arr, size=9, replace=False), arr[b.choice(len(arr), size=9, replace=False)])
    assert np.array_equal(np.unique(a.choice(arr, size=45, replace=True)), arr[np.unique(b.choice(len(arr), size=45, replace=True))])
    assert a.rand() == b.rand()
    counts = np.array([[int(np.sum(l == v)) for v in sir.LABEL_VALUES if v not in sir.IGNORED] for l in labels], np.int64)
    out['class_counts'] = counts
    for e, (steps, batch_num) in enumerate(EPOCHS):
        n_centres = steps * batch_num
        c = Cfg()
        c.epoch_steps, c.batch_num = steps, batch_num
        ds = types.SimpleNamespace(use_potentials=False, epoch_i=torch.zeros(1, dtype=torch.int64), config=c, set='training',
                                   epoch_inds=None, num_clouds=len(labels), input_labels=labels,
                                   label_values=sir.LABEL_VALUES, ignored_labels=np.array(sir.IGNORED))
        seed = 18800 + e
        ours = sir.epoch_draw(labels, sir.LABEL_VALUES, sir.IGNORED, sir.NUM_CLASSES, n_centres, np.random.RandomState(seed))
        ds.epoch_inds = torch.zeros((2, ours.shape[1]), dtype=torch.int64)
        smp = Vaihingen3DPLSampler.__new__(Vaihingen3DPLSampler)
        smp.dataset, smp.N = ds, steps
        np.random.seed(seed)
        next(iter(smp))
        ref_next = np.random.rand()
        ref_inds = ds.epoch_inds.numpy()
        assert np.array_equal(ref_inds, ours), "(r1) the restatement differs from the reference's __iter__"
        rs = np.random.RandomState(seed)
        tri = draw_epoch_positions(counts, n_centres, rs)
        assert rs.rand() == ref_next, "(r1) the position draw leaves the stream elsewhere"
        values = [v for v in sir.LABEL_VALUES if v not in sir.IGNORED]
        pos_inds = np.array([[t[0] for t in tri], [np.where(labels[t[0]] == values[t[1]])[0][t[2]] for t in tri]], np.int64)
        assert np.array_equal(pos_inds, ref_inds), "(r1) the position draw differs from the reference's __iter__"
        out['epoch%d/inds' % e], out['epoch%d/seed' % e] = ref_inds, np.int64(seed)
        out['epoch%d/steps' % e], out['epoch%d/batch_num' % e] = np.int64(steps), np.int64(batch_num)
        out['epoch%d/next_rand' % e], out['epoch%d/triples' % e] = np.float64(ref_next), tri
        pick_n = int(np.ceil(n_centres / (len(labels) * sir.NUM_CLASSES)))
        kinds = {('all' if m <= pick_n else 'some' if m < 50 * pick_n else 'many') for m in counts.reshape(-1)}
        assert kinds == {'all', 'some', 'many'} and (counts == 0).any(), (pick_n, counts)
        print("epoch", e, "pick_n", pick_n, "centres", ref_inds.shape[1], "of", n_centres)
    # ranks 0 and count - 1 are picked (dense class 7, all three taken), a class sits inside one chunk (dense class 6)
    tri = out['epoch0/triples']
    c7 = tri[(tri[:, 0] == 1) & (tri[:, 1] == 6)]
    assert sorted(c7[:, 2].tolist()) == [0, 1, 2] and counts[1, 6] == 3 and out['epoch0/inds'].shape[1] <= 48
    n = len(labels[1])
    gn = -(-n // 256)
    per = -(-n // gn)
    idx = np.where(labels[1] == 6)[0]
    assert n % 256 != 0 and len(idx) == 40 and idx[0] // per == idx[-1] // per and counts[0, 5] == 0
    assert (tri[:, 0] == 1).any() and ((tri[:, 0] == 1) & (tri[:, 1] == 5)).any()


def main():
    out = {}
    cfg = Cfg()
    clouds = sir.scene()
    lut = label_lut(sir.LABEL_VALUES)
    pot_points = [sir.potential_points(p, sir.IN_RADIUS) for p, _, _ in clouds]
    rs = np.random.RandomState(18)
    pots0 = [rs.rand(len(p)) * 1e-3 for p in pot_points]
    pots0[0] *= 0.01                  # so that the sparse cloud, twenty times fewer potential points, takes a turn too
    out.update(in_radius=np.float64(sir.IN_RADIUS), dl=np.float64(sir.DL), batch_limit=np.int64(sir.BATCH_LIMIT),
               max_spheres=np.int64(sir.MAX_SPHERES), clouds=np.array(sir.CLOUDS, np.float64), label_values=sir.LABEL_VALUES,
               ignored=np.array(sir.IGNORED, np.int64), lut=lut, augment_color=np.float64(cfg.augment_color))
    for i, (p, l, c) in enumerate(clouds):
        out['sub_sha_%d' % i], out['sub_n_%d' % i] = digest(p), np.int64(len(p))
        out['labels_sha_%d' % i], out['colors_sha_%d' % i] = digest(l), digest(c)
        out['pot_points_sha_%d' % i] = digest(pot_points[i])
        out['pots0_%d' % i] = pots0[i]
        print("cloud", i, len(p), "sub-points,", len(pot_points[i]), "potential points")
    labels = [l for _, l, _ in clouds]
    pin_epoch_draw(cfg, labels, out)
    pin_items(cfg, clouds, lut, pot_points, pots0, out['epoch0/inds'])
    closest = np.inf
    # four chained potential batches with colours
    ref = sir.RefItems(clouds, sir.IN_RADIUS, pot_points, pots0)
    kept_flags = set()
    for b in range(NB):
        seeds = 18000 + b * sir.MAX_SPHERES + np.arange(sir.MAX_SPHERES)
        d = slot_draws(cfg, seeds)
        res = ref.batch(d, sir.MAX_SPHERES, sir.BATCH_LIMIT, fd=4, lut=lut)
        closest = min(closest, check_membership(clouds, res))
        kept_flags |= {int(d['colour_keep'][k]) for k in res['slots']}
        for key in ('noise', 'R', 'scale', 'colour_keep'):
            out['b%d/draws_%s' % (b, key)] = d[key]
        store(out, 'b%d' % b, res, ref, full=(b == 0))
        print("potential batch", b, res['lengths'], res['cloud_inds'], d['colour_keep'][res['slots']])
    assert kept_flags == {0, 1}, "the kept slots must hold a dropped and a kept colour"
    assert {int(c) for b in range(NB) for c in out['b%d/cloud_inds' % b]} == {0, 1}, "both clouds must be sampled"
    # random_item: three chained batches from epoch 0's list, then one whose slot 1 is lifted 50 units above its cloud
    rnd = sir.RefItems(clouds, sir.IN_RADIUS)
    rnd.epoch_inds = out['epoch0/inds']
    for b in range(3):
        seeds = 18300 + b * sir.MAX_SPHERES + np.arange(sir.MAX_SPHERES)
        d = slot_draws(cfg, seeds)
        res = rnd.batch(d, sir.MAX_SPHERES, sir.BATCH_LIMIT, fd=4, lut=lut, random=True)
        closest = min(closest, check_membership(clouds, res))
        for key in ('noise', 'R', 'scale', 'colour_keep'):
            out['r%d/draws_%s' % (b, key)] = d[key]
        store(out, 'r%d' % b, res)
        out['r%d/epoch_i' % b] = np.int64(rnd.epoch_i)
        print("random batch", b, res['lengths'], res['cloud_inds'], "epoch_i", rnd.epoch_i)
    d = slot_draws(cfg, 18400 + np.arange(sir.MAX_SPHERES))
    d['noise'][1] = [0.0, 0.0, 50.0]
    res = rnd.batch(d, sir.MAX_SPHERES, sir.BATCH_LIMIT, fd=4, lut=lut, random=True)
    assert res['n_fail'] == 1 and len(res['lengths']) >= 2 and rnd.epoch_i == out['r2/epoch_i'] + len(res['lengths']) + 1
    closest = min(closest, check_membership(clouds, res))
    for key in ('noise', 'R', 'scale', 'colour_keep'):
        out['rdrop/draws_%s' % key] = d[key]
    store(out, 'rdrop', res)
    out['rdrop/epoch_i'] = np.int64(rnd.epoch_i)
    out['closest_rel'] = np.float64(closest)
    path = os.path.join(HERE, "g18_sampler_items.npz")
    np.savez_compressed(path, **out)
    print("wrote g18_sampler_items.npz %.1f kB, closest point to a sphere's surface (relative): %.3g" % (os.path.getsize(path) / 1e3, closest))
    assert os.path.getsize(path) <= 558000


if __name__ == "__main__":
    main()
