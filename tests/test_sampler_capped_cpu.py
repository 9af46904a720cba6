"""CPU (no GPU needed): the conditions that keep tests/test_sampler_capped_gpu.py from passing vacuously, asserted on
tests/sampler_ref.py alone.  The scene (tests/sampler_capped_scene.py) is meant to put every chunk of csrc/sampler.hip into
its second and third trip, to hold a tile smaller than the grid, and to start from potentials full of ties; whether it
does is a property of its seeds.  Seeds tried: SEED_A = 4101, SEED_B = 4102, SEED_DRAWS = 4110 -- the first ones tried, and
the reference meets every condition below with them."""
import numpy as np

import sampler_capped_scene as cs


def test_the_capped_scene_meets_the_conditions_of_its_gpu_tests():
    s = cs.scene()
    # sizes: three trips and more in every chunk of tile A, tile B below both grids
    assert cs.N_A > 524288 and s.p_a > 262144 and (s.gp, s.gn) == (cs.GP_CAP, cs.GN_CAP) == (256, 1024)
    assert s.per_n >= 513 and s.per_p >= 513
    assert cs.N_B < s.gn and s.p_b < s.gp // 2 and cs.per(cs.N_B, s.gn) == 1 and cs.per(s.p_b, s.gp) == 1
    for (p, l), n in zip(s.clouds, (cs.N_A, cs.N_B)):
        assert p.dtype == np.float32 and p.shape == (n, 3) and l.dtype == np.int32 and l.shape == (n,)
    # the ties: the smaller index in a third trip, the larger in the first trip of a later chunk
    assert s.tie_first < s.tie_second and s.tie_first // s.per_p < s.tie_second // s.per_p
    assert cs.trips([s.tie_first, s.tie_second], s.p_a, s.gp).tolist() == [2, 0]
    pot_a, pot_b = s.pots0
    assert np.count_nonzero(pot_a != cs.POT_A) == 2 and pot_a[s.tie_first] == pot_a[s.tie_second] == cs.POT_MIN
    assert (pot_b == cs.POT_B).all() and cs.POT_MIN < cs.POT_B < cs.POT_A
    # labels of tile A: three 7s (first point, a third trip of a middle chunk, last point), no 6, a run of 5 over a boundary
    lab = s.clouds[0][1]
    sevens = np.nonzero(lab == 7)[0]
    assert sevens.tolist() == [0, 500 * s.per_n + 550, cs.N_A - 1] and cs.trips(sevens, cs.N_A, s.gn)[1] == 2
    assert not (lab == 6).any() and not (s.clouds[1][1] == 6).any()
    fives = np.nonzero(lab == 5)[0]
    assert len(fives) == cs.RUN_5 and (np.diff(fives) == 1).all() and fives[0] // s.per_n + 1 == fives[-1] // s.per_n
    assert set(cs.trips(fives, cs.N_A, s.gn).tolist()) == {0, 1, 2}
    assert {5, 7} <= set(s.clouds[1][1].tolist())

    chain, failed = cs.reference_chain()
    assert failed == 1 and [w['n_fail'] for w, _ in chain] == [1, 0]                # exactly one sphere is dropped
    first = chain[0][0]
    assert cs.DROP_SLOT not in first['slots'] and len(first['slots']) == cs.MAX_SPHERES - 1
    clouds = np.concatenate([w['cloud_inds'] for w, _ in chain])
    points = np.concatenate([w['point_inds'] for w, _ in chain])
    assert (clouds == 0).sum() >= 2 and (clouds == 1).sum() >= 1
    assert clouds[:2].tolist() == [0, 0] and points[:2].tolist() == [s.tie_first, s.tie_second]      # the tie, in index order
    moved = np.nonzero(clouds == 1)[0]
    assert moved[0] == 2 and (clouds[moved[-1] + 1:] == 0).all() and len(clouds) > moved[-1] + 1      # to B and back to A
    for w, _ in chain:
        assert w['lengths'].sum() <= cs.BATCH_LIMIT                                 # the stop rule never cut a batch
        for sl, c in zip(cs.sphere_slices(w['lengths']), w['cloud_inds']):
            inds = w['input_inds'][sl]
            assert (np.diff(inds) > 0).all()
            if c == 0:                                                              # members in all three trips
                t = np.bincount(cs.trips(inds, cs.N_A, s.gn), minlength=3)
                assert len(t) == 3 and t.min() >= 1, t
    # back on A the arg-min is the first index no sphere has touched, among equal values
    pot_after = chain[1][1][0]
    untouched = np.nonzero(pot_after == cs.POT_A)[0]
    assert len(untouched) > 200000 and int(np.argmin(pot_after)) == untouched[0]
