"""GPU: csrc/sampler.hip ABOVE its grid caps (WS_SAMPLER_GP = 256 workgroups over the potential points, WS_SAMPLER_GN = 1024
over the cloud's points) and on a tile smaller than the grid, against tests/sampler_ref.py, tests/sampler_items_ref.py and
numpy on the scene of tests/sampler_capped_scene.py.  The goldens g15 / g18 stay below 256 items per chunk; here a workgroup
walks its chunk in three trips and more and carries state across them: `local += tot` (sphere_emit_kernel), `r -= tot`
with the early break (class_select_kernel), the strided count, arg-min and Tukey loops.  Integers are compared for
equality and floats bit for bit: no tolerance anywhere.  tests/test_sampler_capped_cpu.py holds the scene to the
conditions without which these tests would pass vacuously."""
import numpy as np
import pytest
import torch

import sampler_capped_scene as cs
import sampler_items_ref as sir
from test_sampler_gpu import as_numpy, assert_same_batch, bits_equal

pytestmark = pytest.mark.gpu
ROOMY = 16384                                                  # rows: above what 8 spheres of the scene hold


@pytest.fixture(scope="module")
def capped():
    return cs.scene()


def make_sampler(s, dev, use_potentials=True, **kw):
    from weasal_amd.sampler import SphereSampler
    kw.setdefault('max_spheres', cs.MAX_SPHERES)
    kw.setdefault('seed', 3)
    sm = SphereSampler(cs.Cfg(), [(torch.from_numpy(p).to(dev), torch.from_numpy(l).to(dev)) for p, l in s.clouds],
                       label_values=cs.LABEL_VALUES, ignored_labels=cs.IGNORED, batch_limit=cs.BATCH_LIMIT,
                       use_potentials=use_potentials, **kw)
    if use_potentials:
        for got, want in zip(sm.pot_points, s.pot_points):    # the HIP grid subsampling equals the CPU oracle's
            assert bits_equal(got.cpu().numpy(), want)
        sm.set_potentials(s.pots0)
    return sm


def assert_equals_reference(got, want, tag):
    assert got['labels'].dtype == np.int64 and got['input_inds'].dtype == np.int64 and got['lengths'].dtype == np.int32
    for k in ('lengths', 'cloud_inds', 'point_inds', 'input_inds', 'labels'):
        assert np.array_equal(got[k], want[k]), (tag, k)
    for k in ('points', 'features', 'scales', 'rots'):
        assert bits_equal(got[k], want[k]), (tag, k)


def report(tag, s, got):
    """the log line that shows the capped paths ran: members of the spheres on tile A seen in second and later trips"""
    second = third = 0
    for sl, c in zip(cs.sphere_slices(got['lengths']), got['cloud_inds']):
        inds = got['input_inds'][sl]
        assert (np.diff(inds) > 0).all(), (tag, "input_inds must ascend inside every sphere")
        if c == 0:
            a, b = cs.trip_counts(inds, cs.N_A, s.gn)
            second, third = second + a, third + b
    print("%s: gn = %d, gp = %d, per = %d (potential chunks %d), members of tile A in second trips %d, in third trips %d"
          % (tag, s.gn, s.gp, s.per_n, s.per_p, second, third))
    return second, third


def test_two_chained_batches_above_the_caps_equal_the_cpu_restatement(gpu, capped):
    s = capped
    chain, failed = cs.reference_chain()
    sm = make_sampler(s, gpu)
    seen = np.zeros(2, np.int64)
    for b, (want, want_pots) in enumerate(chain):
        got = as_numpy(sm.sample(draws=cs.draws(b), capacity_rows=ROOMY))
        assert_equals_reference(got, want, b)
        pots = [p.cpu().numpy() for p in sm.potentials]
        for i in range(2):
            assert bits_equal(pots[i], want_pots[i]), (b, i)
        assert bits_equal(sm.last_centres, want['centres'])
        assert np.array_equal(sm.lengths_dev.cpu().numpy(), got['lengths'])
        seen += report("chained batch %d" % b, s, got)
    assert seen.min() > 0
    assert sm.failed == failed == 1 and sm._sync_count == 2
    head, slots = sm.last_state
    assert head['attempts'] == cs.MAX_SPHERES


def test_capacity_retry_resumes_with_carried_counts(gpu, capped):
    s = capped
    want, want_pots = cs.reference_chain()[0][0]
    d = cs.draws(0)
    roomy = make_sampler(s, gpu)
    full = as_numpy(roomy.sample(draws=d, capacity_rows=ROOMY))
    assert roomy._sync_count == 1
    assert_equals_reference(full, want, "roomy")
    cap = int(full['lengths'][:3].sum()) - 1                   # the third sphere (the first on tile B) does not fit
    sm = make_sampler(s, gpu)
    got = as_numpy(sm.sample(draws=d, capacity_rows=cap))
    assert sm._sync_count >= 2, "the small buffer must have been noticed"
    assert_same_batch(got, full)
    for p, q, w in zip(sm.potentials, roomy.potentials, want_pots):
        assert bits_equal(p.cpu().numpy(), q.cpu().numpy()) and bits_equal(p.cpu().numpy(), w)
    assert sm.seq == roomy.seq and sm.failed == roomy.failed == 1
    assert min(report("capacity retry at %d rows" % cap, s, got)) > 0


def test_set_erf_walks_the_potentials_and_leaves_them_alone(gpu, capped):
    """update_pot = 0: the strided arg-min of sphere_scan_kernel runs on the stored potentials, nothing is written"""
    s = capped
    d = cs.draws(1)                                            # no lifted slot
    sm = make_sampler(s, gpu, set='ERF')
    got = as_numpy(sm.sample(draws=d, capacity_rows=ROOMY))
    for p, w in zip(sm.potentials, s.pots0):
        assert bits_equal(p.cpu().numpy(), w)
    ref = cs.ref_sampler(s)
    want = ref.batch(d, cs.MAX_SPHERES, cs.BATCH_LIMIT, fd=3, labels_zero=True, update=False)
    assert_equals_reference(got, want, "ERF")
    assert len(got['lengths']) == cs.MAX_SPHERES and (got['point_inds'] == s.tie_first).all() and not got['labels'].any()
    assert bits_equal(sm.last_centres, want['centres']) and sm.failed == 0
    assert min(report("set ERF", s, got)) > 0


def test_random_mode_centres_in_the_first_a_middle_and_the_last_chunk(gpu, capped):
    """use_potentials=False: gp = 0, workgroup b is chunk b"""
    s = capped
    p = s.per_n
    centres = [(0, 5), (0, 512 * p + 300), (1, 350), (0, cs.N_A - 3), (0, 77 * p + 585), (1, 0), (0, 1023 * p), (0, 300 * p - 1),
               (1, 699), (0, 9), (0, 10)]
    epoch_inds = np.array(centres, np.int64).T.copy()
    assert epoch_inds[1, 3] // p == s.gn - 1 and epoch_inds[1, 0] // p == 0
    sm = make_sampler(s, gpu, use_potentials=False)
    assert sm.potentials == [] and sm.pot_points == []
    sm.set_epoch_inds(epoch_inds)
    d = cs.draws(1)
    got = as_numpy(sm.sample(draws=d, capacity_rows=ROOMY))
    ref = sir.RefItems(s.clouds, cs.IN_RADIUS)
    ref.epoch_inds, ref.epoch_i = epoch_inds, 0
    want = ref.batch(d, cs.MAX_SPHERES, cs.BATCH_LIMIT, fd=3, lut=cs.LABEL_VALUES, random=True)
    assert_equals_reference(got, want, "random")
    assert bits_equal(sm.last_centres, want['centres'])
    assert int(sm.epoch_i.item()) == ref.epoch_i == cs.MAX_SPHERES and sm.failed == ref.failed == 0
    assert got['cloud_inds'].tolist() == [c for c, _ in centres[:8]] and got['point_inds'].tolist() == [i for _, i in centres[:8]]
    second, third = report("random mode", s, got)
    assert min(second, third) > 0
    print("random mode: gp = 0 in this launch (no workgroup over the potential points)")


def test_noise_of_later_trip_rows_is_a_pure_function_of_its_key(gpu, capped):
    s = capped
    d = cs.draws(0)
    sigma = 0.05

    def run(max_spheres, noise=sigma):
        sm = make_sampler(s, gpu, max_spheres=max_spheres, seed=7)
        return as_numpy(sm.sample(draws=d, augment_noise=noise, capacity_rows=ROOMY))
    a, b = run(cs.MAX_SPHERES), run(cs.MAX_SPHERES)
    assert_same_batch(a, b)                                    # same (seed, seq): same bits
    zero = run(cs.MAX_SPHERES, noise=0.0)
    assert bits_equal(a['input_inds'], zero['input_inds']) and bits_equal(a['lengths'], zero['lengths'])
    moved = (a['points'] != zero['points']).any(axis=1)
    assert moved.mean() > 0.99
    # a chain cut after sphere slot 1 (two spheres on A) and after slot 5 (A, A, B, dropped, B, A): the rows of every sphere
    # carry the noise of the same (sphere sequence number, row in the sphere) as in the chain of 8
    for cut in (2, 6):
        c = run(cut)
        kept = len(c['lengths'])
        rows = int(c['lengths'].sum())
        assert kept == cut - (1 if cut > cs.DROP_SLOT else 0) and np.array_equal(c['lengths'], a['lengths'][:kept])
        for k in ('points', 'features', 'labels', 'input_inds'):
            assert bits_equal(c[k], a[k][:rows]), (cut, k)
        for k in ('scales', 'rots', 'cloud_inds', 'point_inds'):
            assert bits_equal(c[k], a[k][:kept]), (cut, k)
    later = np.concatenate([cs.trips(a['input_inds'][sl], cs.N_A, s.gn) >= 1 if cl == 0 else np.zeros(sl.stop - sl.start, bool)
                            for sl, cl in zip(cs.sphere_slices(a['lengths']), a['cloud_inds'])])
    assert moved[later].mean() > 0.99
    assert min(report("noise", s, a)) > 0


# ---------------------------------------------------------------------------------------------------------------
# the class-balanced centre draw
# ---------------------------------------------------------------------------------------------------------------
def test_class_counts_and_select_above_the_caps(gpu, capped):
    s = capped
    labels = [l for _, l in s.clouds]
    values = np.array([v for v in cs.LABEL_VALUES if v not in cs.IGNORED], np.int32)
    sm = make_sampler(s, gpu, use_potentials=False)
    d_values = torch.from_numpy(values).to(gpu)
    d_counts = torch.empty((2, len(values)), dtype=torch.int64, device=gpu)
    sm.handle.class_counts(d_values, d_counts)
    counts = d_counts.cpu().numpy()
    want_counts = np.array([[(l == v).sum() for v in values] for l in labels], np.int64)
    assert np.array_equal(counts, want_counts)
    cls = {int(v): i for i, v in enumerate(values)}
    assert counts[0, cls[7]] == 3 and counts[0, cls[6]] == counts[1, cls[6]] == 0 and counts[0, cls[5]] == cs.RUN_5
    rs = np.random.RandomState(4120)
    triples = []
    for cloud in range(2):
        for v in (5, 7):                                       # every position, then the count itself and far past it
            m = int(want_counts[cloud, cls[v]])
            triples += [(cloud, cls[v], pos) for pos in list(range(m)) + [m, m + 1, 10 ** 12]]
        triples += [(cloud, cls[6], 0), (cloud, cls[6], 5)]    # an absent class
    big = [cls[v] for v in (1, 2, 3, 4, 8)]
    for c in big:
        m = int(want_counts[0, c])
        assert m > 50000
        triples += [(0, c, int(pos)) for pos in rs.randint(0, m, size=2000)]
        triples += [(0, c, 0), (0, c, m - 1), (0, c, m), (0, c, 2 * cs.N_A)]
    triples += [(2, 0, 0), (-1, 0, 0), (0, len(values), 0), (0, -1, 0), (0, cls[1], -1), (1, 64, 3)]     # outside the tables
    triples = np.array(triples, np.int64)
    out = torch.empty(len(triples), dtype=torch.int64, device=gpu)
    sm.handle.class_select(d_values, torch.from_numpy(triples).to(gpu), out)
    got = out.cpu().numpy()
    members = {(cloud, c): np.nonzero(labels[cloud] == values[c])[0] for cloud in range(2) for c in range(len(values))}
    want = np.full(len(triples), -1, np.int64)
    for t, (cloud, c, pos) in enumerate(triples):
        if 0 <= cloud < 2 and 0 <= c < len(values) and 0 <= pos < len(members[(cloud, c)]):
            want[t] = members[(cloud, c)][pos]
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(triples[t].tolist(), int(got[t]), int(want[t])) for t in bad[:8]]
    assert (want == -1).sum() >= 6 + 3 * 4 + 4 + 2 * len(big)
    on_a = want[(triples[:, 0] == 0) & (want >= 0)]
    second, third = cs.trip_counts(on_a, cs.N_A, s.gn)
    print("class select: gn = %d, gp = 0, per = %d, %d triples, selected members of tile A in second trips %d, in third trips %d"
          % (s.gn, s.per_n, len(triples), second, third))
    assert min(second, third) > 0


@pytest.mark.parametrize("n_steps", [8, 12])                   # pick_n = 2 and 3
def test_epoch_draw_above_the_caps_equals_the_references_iter(gpu, capped, n_steps):
    s = capped
    labels = [l for _, l in s.clouds]
    n_centres = n_steps * cs.Cfg.batch_num
    assert int(np.ceil(n_centres / (2 * cs.NUM_CLASSES))) == {8: 2, 12: 3}[n_steps]
    sm = make_sampler(s, gpu, use_potentials=False)
    sm.rng = np.random.RandomState(4130 + n_steps)
    reads = sm._epoch_sync_count
    inds = sm.draw_epoch_centres(n_steps)
    assert sm._epoch_sync_count - reads == 1 and inds.dtype == torch.int64 and int(sm.epoch_i.item()) == 0
    rng = np.random.RandomState(4130 + n_steps)
    want = sir.epoch_draw(labels, cs.LABEL_VALUES, cs.IGNORED, cs.NUM_CLASSES, n_centres, rng)
    got = inds.cpu().numpy()
    assert np.array_equal(got, want)
    assert sm.rng.rand() == rng.rand()                         # both streams were consumed alike
    assert np.array_equal(sm.last_class_counts, [[(l == v).sum() for v in cs.LABEL_VALUES[1:]] for l in labels])
    second, third = cs.trip_counts(got[1][got[0] == 0], cs.N_A, s.gn)
    print("epoch draw at pick_n = %d: gn = %d, gp = 0, per = %d, %d centres, on tile A in second trips %d, in third trips %d"
          % (int(np.ceil(n_centres / 16)), s.gn, s.per_n, got.shape[1], second, third))
    assert second + third > 0
