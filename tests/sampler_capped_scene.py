"""The scene of the sphere sampler's tests ABOVE its grid caps (helper of test_sampler_capped_cpu.py, test_sampler_capped_gpu.py
and test_tester.py; no tests in it).  Everything is built from fixed RandomState seeds; nothing is read from a file.

csrc/sampler.hip gives the potential points at most GP_CAP = 256 workgroups and the cloud's points at most GN_CAP = 1024;
workgroup b owns `chunk(n, blocks, b)` = [b * per, (b + 1) * per) with per = ceil(n / blocks) and walks it in trips of 256.
Tile A is large enough for three trips and more in every chunk of both kinds, tile B is smaller than either grid:

  tile A   N_A = 600 000 uniform float32 points in a slab 45 x 45 x 0.2 (the density of a 32 x 32 slab with 300 000 points:
           293 points per unit of ground, about 920 in a sphere of radius 1 away from the border), per = 586: trips
           [0, 256), [256, 512), [512, 586).  Its potential points (sampler_ref.potential_points at in_radius / 10) are more
           than 262 144, so a potential chunk has more than 1 024 points: five trips.
  tile B   N_B = 700 points in a strip 1.2 x 0.06 x 0.2: per = 1, 324 of the 1 024 chunks are empty; about 48 potential
           points, so most of the 256 potential chunks are empty too.

Labels of tile A (section "class-balanced centre draw" of the tests): 7 has exactly three members -- index 0, an index in the
third trip of a middle chunk, N_A - 1 --, 6 is absent, 5 is a run of 600 consecutive points across a chunk boundary, the
others are random.  Tile B: random among every value but 6.

Start potentials: tile A is the constant POT_A but for two equal strict minima POT_MIN, the smaller index TIE_FIRST in the
third trip of potential chunk 100, the larger TIE_SECOND in the first trip of chunk 180; tile B is the constant POT_B
between the two.  A chain therefore takes the tie to the first index, then the second, moves to B until B's potentials
have risen above POT_A, and comes back to A, where the arg-min is the first untouched index among equal values.

Draws: sampler.draw_slots with the configuration below; slot DROP_SLOT of the first batch lifts its centre 5 above the
slab, so its sphere is empty and is dropped.
"""
import functools

import numpy as np

import sampler_ref

IN_RADIUS = 1.0
BLOCK, GP_CAP, GN_CAP = 256, 256, 1024                        # csrc/sampler.hip: threads, WS_SAMPLER_GP, WS_SAMPLER_GN
N_A, HALF_A, ZHALF = 600000, 22.5, 0.1
N_B, HALF_BX, HALF_BY = 700, 0.6, 0.03
SEED_A, SEED_B, SEED_DRAWS = 4101, 4102, 4110
MAX_SPHERES, BATCH_LIMIT, DROP_SLOT = 8, 50000, 3             # the limit is never reached: every batch runs its 8 slots
POT_A, POT_B, POT_MIN = 0.5, 0.3, 0.1
LABEL_VALUES = np.arange(9, dtype=np.int64)
IGNORED = (0,)
NUM_CLASSES = 8
RUN_5 = 600                                                   # length of the run of label 5


class Cfg:
    """GoldenCfg of test_sampler_gpu.py at in_radius 1"""
    in_features_dim = 3
    in_radius = IN_RADIUS
    augment_rotation = 'vertical'
    augment_scale_anisotropic = True
    augment_scale_min = 0.9
    augment_scale_max = 1.1
    augment_symmetries = [True, False, False]
    augment_noise = 0.0
    batch_num = 4
    epoch_steps = 12
    validation_size = 7
    num_classes = NUM_CLASSES


def grid(nmax, pmax):
    """(gp, gn) of ws_sampler_batch_items for tiles of at most nmax points and pmax potential points"""
    return min(-(-pmax // BLOCK), GP_CAP), min(-(-nmax // BLOCK), GN_CAP)


def per(n, blocks):
    return -(-n // blocks)


def trips(inds, n, blocks):
    """trip of its chunk's walk in which every index is visited"""
    return (np.asarray(inds) % per(n, blocks)) // BLOCK


def trip_counts(inds, n, blocks):
    """-> (members seen in a second trip, in a third or later trip)"""
    t = trips(inds, n, blocks)
    return int((t == 1).sum()), int((t >= 2).sum())


def _slab(seed, n, hx, hy, hz):
    rs = np.random.RandomState(seed)
    return np.ascontiguousarray((rs.uniform(-1.0, 1.0, size=(n, 3)) * np.array([hx, hy, hz])).astype(np.float32))


def labels_a():
    rs = np.random.RandomState(SEED_A + 1000)
    lab = rs.choice(np.array([0, 1, 2, 3, 4, 8], np.int32), size=N_A).astype(np.int32)
    p = per(N_A, GN_CAP)
    start = 300 * p - 250                                     # 250 points in chunk 299 (all three trips of its tail), 350 in chunk 300
    lab[start:start + RUN_5] = 5
    lab[[0, 500 * p + 550, N_A - 1]] = 7
    return lab


def labels_b():
    rs = np.random.RandomState(SEED_B + 1000)
    return rs.choice(np.array([0, 1, 2, 3, 4, 5, 7, 8], np.int32), size=N_B).astype(np.int32)


def draws(batch):
    """the DRAW_DTYPE records of the 8 slots of chained batch 0 or 1"""
    from weasal_amd.sampler import draw_slots
    d, _ = draw_slots(Cfg(), np.random.RandomState(SEED_DRAWS + batch), MAX_SPHERES)
    if batch == 0:
        d['noise'][DROP_SLOT] = (0.0, 0.0, 5.0)
    return d


class Scene:
    pass


@functools.lru_cache(maxsize=1)
def scene():
    """-> Scene: clouds [(points, labels)] of A and B, pot_points, pots0, the grid, the two tie indices"""
    s = Scene()
    s.clouds = [(_slab(SEED_A, N_A, HALF_A, HALF_A, ZHALF), labels_a()), (_slab(SEED_B, N_B, HALF_BX, HALF_BY, ZHALF), labels_b())]
    s.pot_points = [sampler_ref.potential_points(p, IN_RADIUS) for p, _ in s.clouds]
    s.p_a, s.p_b = (len(p) for p in s.pot_points)
    s.gp, s.gn = grid(N_A, s.p_a)
    s.per_n, s.per_p = per(N_A, s.gn), per(s.p_a, s.gp)
    s.tie_first, s.tie_second = 100 * s.per_p + 600, 180 * s.per_p + 10
    pot_a = np.full(s.p_a, POT_A, np.float64)
    pot_a[[s.tie_first, s.tie_second]] = POT_MIN
    s.pots0 = [pot_a, np.full(s.p_b, POT_B, np.float64)]
    return s


def ref_sampler(s):
    return sampler_ref.RefSampler(s.clouds, s.pot_points, s.pots0, IN_RADIUS)


@functools.lru_cache(maxsize=1)
def reference_chain():
    """the two chained batches of RefSampler on the scene -> [(outputs, potentials after the batch)], failed"""
    s = scene()
    ref = ref_sampler(s)
    out = []
    for b in range(2):
        want = ref.batch(draws(b), MAX_SPHERES, BATCH_LIMIT, fd=3, lut=LABEL_VALUES)
        out.append((want, [p.copy() for p in ref.potentials]))
    return out, ref.failed


def sphere_slices(lengths):
    offs = np.cumsum(lengths) - lengths
    return [slice(int(o), int(o + n)) for o, n in zip(offs, lengths)]
