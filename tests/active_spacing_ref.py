"""CPU restatement (numpy, float64) of the active-learning selection with a minimum spacing ("spaced greedy"), the
yardstick of tests/test_active_spacing_*.py; nothing here touches the device library.

Contract: walk the candidates in the priority order of the plain selection (active_ref.order with the used ids removed:
descending score, ascending index among equal scores, -0.0 == +0.0, NaN last); accept a candidate iff no id accepted before
it and no used id blocks it; stop after k acceptances; the accepted ids in acceptance order.  q blocks p iff d2 < s * s,
strict, the coordinates widened to float64, d2 = (dx*dx + dy*dy) + dz*dz with every operation rounded on its own (numpy
fuses nothing), s * s formed in float64.  Fewer than k acceptances: ValueError with the reference's message and the spacing.

`WRONG` is a tuple of plausible mistakes; the CPU test requires each to differ from the restatement on some row of `rows()`,
so that a device result equal to the restatement cannot be one of them.
"""
import numpy as np

import active_ref

POINT_MESSAGE = 'Not enough point labels left for the next iteration'
ANCHOR_MESSAGE = 'Not enough weak labels left for the next iteration'


def d2_to(coords, q, dtype=np.float64, dims=3):
    """squared distance of every row of coords to the point q, (dx*dx + dy*dy) + dz*dz in `dtype`"""
    c = np.asarray(coords).astype(dtype)
    d = c - np.asarray(q).astype(dtype)
    out = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    return out + d[:, 2] * d[:, 2] if dims == 3 else out


def priority(score, used, ties_descending=False):
    """the candidates in walk order"""
    s = np.asarray(score, np.float64)
    if ties_descending:
        ids = s.shape[0] - 1 - active_ref.order(s[::-1])
    else:
        ids = active_ref.order(s)
    keep = np.ones(s.shape[0], bool)
    keep[np.asarray(used, np.int64)] = False
    return ids[keep[ids]]


def walk(score, coords, used, k, spacing, message=POINT_MESSAGE, strict=True, used_block=True, ties_descending=False,
         dtype=np.float64, dims=3, stop_at_candidates=False):
    """-> (ids int64 [<= k], position in the candidate list just behind the last acceptance).  The keywords are the
    mistakes of WRONG; the defaults are the contract."""
    coords = np.asarray(coords)
    s2 = dtype(np.float64(spacing) * np.float64(spacing)) if dtype is np.float64 else dtype(spacing) * dtype(spacing)
    blocked = np.zeros(coords.shape[0], bool)
    near = (lambda d2: d2 < s2) if strict else (lambda d2: d2 <= s2)
    if used_block:
        for u in np.unique(np.asarray(used, np.int64)):
            blocked |= near(d2_to(coords, coords[u], dtype, dims))
    cand = priority(score, used, ties_descending)
    if stop_at_candidates:
        cand = cand[:k]
    out, behind = [], 0
    for pos, i in enumerate(cand):
        if len(out) == k:
            break
        if blocked[i]:
            continue
        out.append(i)
        behind = pos + 1
        blocked |= near(d2_to(coords, coords[i], dtype, dims))
    if len(out) < k and not stop_at_candidates:
        raise ValueError('%s (min_spacing %g)' % (message, spacing))
    return np.asarray(out, np.int64), behind


def select(score, coords, used, k, spacing, message=POINT_MESSAGE):
    """the restatement: int64 [k]"""
    return walk(score, coords, used, k, spacing, message)[0]


def acceptable(score, coords, used, spacing):
    """how many ids the walk accepts when it is never stopped"""
    return len(walk(score, coords, used, len(score), spacing, stop_at_candidates=True)[0])


WRONG = (
    ('<= instead of <', dict(strict=False)),
    ('used points do not block', dict(used_block=False)),
    ('ties by descending id', dict(ties_descending=True)),
    ('float32 distance', dict(dtype=np.float32)),
    ('spacing applied to xy only', dict(dims=2)),
    ('stop at k candidates instead of k acceptances', dict(stop_at_candidates=True)),
)


def wrong(name, score, coords, used, k, spacing):
    """the ids of a wrong variant, or the text of its ValueError"""
    try:
        return walk(score, coords, used, k, spacing, **dict(WRONG)[name])[0]
    except ValueError as e:
        return str(e)


# ------------------------------------------------------------------------------------------------------------------
# rows shared by the CPU and the GPU test (the letters are those of the tests' docstrings)
# ------------------------------------------------------------------------------------------------------------------
def _smooth_scores(pts, rng, levels=64):
    """a spatially smooth field (three bumps), quantised to `levels` values: neighbours share a score, ties everywhere"""
    p = pts.astype(np.float64)
    centres = rng.uniform([5, 5, 1], [45, 45, 4], size=(3, 3))
    f = sum(np.exp(-((p - c) ** 2).sum(1) / (2 * 6.0 ** 2)) for c in centres)
    return np.floor(f / f.max() * (levels - 1)) / (levels - 1)


def rows():
    """name -> dict(score f64 [n], coords [n, 3] f32 or f64, used int64, k, spacing, prefix or None)"""
    out = {}
    rng = np.random.default_rng(20240)
    n = 5000
    pts = rng.uniform([0, 0, 0], [50, 50, 5], size=(n, 3)).astype(np.float32)
    score = _smooth_scores(pts, rng)
    top = active_ref.order(score)
    used = np.concatenate([top[rng.choice(400, size=50, replace=False)], rng.choice(n, size=50)]).astype(np.int64)
    out['a'] = dict(score=score, coords=pts, used=used, k=64, spacing=2.0, prefix=None)
    # (b) a lattice whose pitch is the spacing: a neighbour at exactly s is not blocked; and with s = 0.75
    g = np.arange(8, dtype=np.float32) * np.float32(0.5)
    lat = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    lat_score = rng.permutation(512).astype(np.float64)
    out['b_0.5'] = dict(score=lat_score, coords=lat, used=np.zeros(0, np.int64), k=512, spacing=0.5, prefix=None)
    out['b_0.75'] = dict(score=lat_score, coords=lat, used=np.zeros(0, np.int64), k=64, spacing=0.75, prefix=None)
    out['c'] = dict(out['a'], score=np.full(n, 0.25))
    sd = score - 1.0                                             # the top level becomes 0: half of it -0.0
    zero = np.flatnonzero(sd == 0.0)
    sd[zero[::2]] = -0.0
    sd[rng.choice(n, size=n // 10, replace=False)] = np.nan
    out['d'] = dict(out['a'], score=sd)
    line = np.zeros((3000, 3), np.float32)
    line[:, 0] = (np.arange(3000) * 0.3).astype(np.float32)
    dec = -np.arange(3000, dtype=np.float64)
    out['e'] = dict(score=dec, coords=line, used=np.zeros(0, np.int64), k=300, spacing=0.5, prefix=None)
    out['e_long'] = dict(out['e'], k=1500)                       # the same chain over every chunk of the walk
    # (f) the 6000 best within s / 2 of one point; the rest spread out
    nf, s = 10000, 2.0
    ball = rng.standard_normal((6000, 3))
    ball *= (rng.random(6000) ** (1 / 3) * 0.49 * s)[:, None] / np.linalg.norm(ball, axis=1)[:, None]
    far = rng.uniform([0, 0, 0], [200, 200, 20], size=(nf - 6000, 3))
    ptf = np.concatenate([ball + [100.0, 100.0, 10.0], far]).astype(np.float32)
    scf = np.concatenate([2.0 + rng.random(6000), rng.random(nf - 6000)])
    perm = rng.permutation(nf)
    out['f'] = dict(score=scf[perm], coords=ptf[perm], used=np.zeros(0, np.int64), k=32, spacing=s, prefix=256)
    # (g) float64 centres: a lattice of anchors and the overlap centres half way between x-neighbours
    a = np.arange(6, dtype=np.float64) * 0.3
    base = np.stack(np.meshgrid(a, a, a[:2], indexing='ij'), -1).reshape(-1, 3)
    mid = base[base[:, 0] < a[-1]] + [0.15, 0.0, 0.0]
    cg = np.concatenate([base, mid])
    out['g'] = dict(score=np.round(rng.random(len(cg)) * 16) / 16, coords=cg, used=rng.choice(len(cg), size=6).astype(np.int64),
                    k=12, spacing=0.3, prefix=None)
    small = rng.uniform(0, 6, size=(200, 3)).astype(np.float32)
    out['h'] = dict(score=np.round(rng.random(200) * 32) / 32, coords=small, used=np.zeros(0, np.int64), k=8, spacing=1.5,
                    prefix=None)
    # (t) pairs at a distance so close to s that float32 arithmetic decides them differently from float64
    s, pairs, cell = 2.0, [], 0
    while len(pairs) < 40:
        p = (rng.uniform(0, 4, size=3) + [10.0 * cell, 0, 0]).astype(np.float32)
        u = rng.standard_normal(3)
        q = (p.astype(np.float64) + u / np.linalg.norm(u) * s).astype(np.float32)
        both = np.stack([p, q])
        if (d2_to(both, p)[1] < s * s) != (d2_to(both, p, np.float32)[1] < np.float32(s) * np.float32(s)):
            pairs += [p, q]
            cell += 1
    out['t'] = dict(score=-np.arange(40, dtype=np.float64), coords=np.stack(pairs), used=np.zeros(0, np.int64), k=20, spacing=s,
                    prefix=None)
    return out


def lattice_anchors(seed, n_points, centres, c=9):
    """(anchor_ptr, anchor_idx, anchor_labels) for `centres`: every anchor a run of 20..60 consecutive point ids"""
    return active_ref.synthetic_anchors(seed, n_points, len(centres), c, lo=20, hi=60)
