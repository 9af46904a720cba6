"""GPU: active-learning selection (weasal_amd.active, csrc/active.hip) against tests/active_ref.py run on the CPU in the same
test.  Integer outputs and the top-k order are compared for equality.  The two float32 entropies (device log2f and numpy's)
may differ in the last bits, which bounds how far a score may move:

    |H_gpu - H_ref| <= 16 * C * 2^-24
      C terms p * log2(p + 1e-12) of magnitude <= 0.531, each a few float32 ulps off, plus the C - 1 roundings of a sum
      <= log2(C): about 5 * C * 2^-24 against exact arithmetic for each side; the bound allows both sides plus margin.

A selection made from scores that differ by at most t can differ from the reference's only among the ids whose score lies
within t of the reference's k-th score s_k.  The selection tests therefore (1) count, from the restatement alone, the ids
inside [s_k - t, s_k + t] and require at most 1 % of k there, so that the band cannot hide a failure, and (2) require every
selected id to score >= s_k - t and every unselected, unused id <= s_k + t in the reference."""
import numpy as np
import pytest
import torch

from conftest import golden

import active_ref
import sampler_ref

C9 = 9
H_TOL = 16 * C9 * 2.0 ** -24
CLASS_W = np.array([0.2, 1.0, 0.4, 1.8, 0.6, 1.4, 0.8, 1.2, 1.6])
N_SYN = 300000


class Votes:
    """what the selection needs of a tester.VoteAccumulator"""

    def __init__(self, probs):
        self.probs = probs


@pytest.fixture(scope="module")
def syn():
    return active_ref.synthetic_votes(5, N_SYN, C9)


def assert_band_selection(ref_score, used, got, k, t):
    """the band rule of the module docstring"""
    n = len(ref_score)
    want = active_ref.select(ref_score, used, k)
    s_k = ref_score[want[-1]]
    free = np.ones(n, bool)
    free[used] = False
    inside = int((free & (ref_score >= s_k - t) & (ref_score <= s_k + t)).sum())
    print("k=%d s_k=%.9g t=%.3g ids inside the band: %d (allowed %d)" % (k, s_k, t, inside, k // 100))
    assert inside <= k // 100, "the fixture has too many scores next to the k-th one for the band rule to mean anything"
    got = np.asarray(got)
    assert got.shape == (k,) and got.dtype == np.int64
    assert len(np.unique(got)) == k, "duplicates"
    assert got.min() >= 0 and got.max() < n
    assert free[got].all(), "a used id was selected"
    assert (ref_score[got] >= s_k - t).all()
    rest = free.copy()
    rest[got] = False
    assert (ref_score[rest] <= s_k + t).all()
    differ = len(np.setdiff1d(got, want))
    print("ids that differ from the reference's selection: %d" % differ)
    assert differ <= inside


# ------------------------------------------------------------------------------------------------------------------
# 1. scores
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("source", ["g11", "synthetic"])
def test_point_scores(gpu, syn, source):
    from weasal_amd import active
    probs = golden("g11_tester.npz")["test_probs"] if source == "g11" else syn
    assert probs.dtype == np.float32 and probs.shape[1] == C9
    unvoted = (probs.sum(1) == 0)
    assert unvoted.any()
    if source == "synthetic":
        assert 0.02 < unvoted.mean() < 0.04
    h_ref, p_ref, s_ref = active_ref.point_scores(probs, CLASS_W)
    h, p, s = active.point_scores(torch.from_numpy(probs).to(gpu), CLASS_W)
    assert h.dtype == torch.float32 and p.dtype == torch.int32 and s.dtype == torch.float64
    h, p, s = h.cpu().numpy(), p.cpu().numpy(), s.cpu().numpy()
    assert np.array_equal(p, np.argmax(probs, axis=1))
    err = np.abs(h.astype(np.float64) - h_ref.astype(np.float64)).max()
    print("%s: max |H_gpu - H_ref| = %.3g (bound %.3g)" % (source, err, H_TOL))
    assert err <= H_TOL
    assert np.array_equal(s, h.astype(np.float64) * np.exp(CLASS_W)[p])         # the product itself is exact float64
    assert (h[unvoted] == 0).all() and (p[unvoted] == 0).all() and (s[unvoted] == 0).all()
    assert not np.signbit(h[unvoted]).any()


# ------------------------------------------------------------------------------------------------------------------
# 2. top-k is exact
# ------------------------------------------------------------------------------------------------------------------
def topk_case(n, seed):
    rng = np.random.default_rng(seed)
    score = (np.round(rng.standard_normal(n) * 256.0) / 64.0).astype(np.float64)    # multiples of 1/64: many ties
    if n >= 1000:
        score[rng.integers(0, n, size=n // 50)] = -0.0
        score[rng.integers(0, n, size=n // 50)] = 0.0
        score[rng.integers(0, n, size=7)] = np.nan
        score[rng.integers(0, n, size=3)] = np.inf
        score[rng.integers(0, n, size=3)] = -np.inf
        ex = rng.integers(0, n, size=n // 10)
        ex = np.concatenate([ex, ex[: len(ex) // 3], np.flatnonzero(np.isnan(score))[:2]])   # duplicates, a NaN among them
        rng.shuffle(ex)
    else:
        ex = np.zeros(0, np.int64)
    return score, ex.astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 1000, 300000, (1 << 21) + 3])
def test_top_k_is_exact(gpu, n):
    from weasal_amd import active
    score, ex = topk_case(n, 100 + n % 97)
    remaining = n - len(np.unique(ex))
    idx = np.arange(n)
    nan = np.isnan(score)
    full = np.lexsort((idx, np.where(nan, 0.0, -score), nan))                      # NaN last, ties by index
    keep = np.ones(n, bool)
    keep[ex] = False
    full = full[keep[full]].astype(np.int64)
    assert len(full) == remaining
    assert np.array_equal(full, active_ref.select(score, ex, remaining))
    s_dev = torch.from_numpy(score).to(gpu)
    ks = sorted({k for k in (1, 200, 5000, remaining) if k <= remaining})
    assert ks
    for k in ks:
        for exclude in ((ex, torch.from_numpy(ex).to(gpu)) if k == ks[0] else (ex,)):       # host and device id lists
            got = active.top_k(s_dev, k, exclude)
            assert got.dtype == torch.int64 and got.is_cuda and got.shape == (k,)
            assert np.array_equal(got.cpu().numpy(), full[:k]), (n, k)
    if n > 1:
        # no exclusions, float32 scores (the anchor case: widened exactly)
        s32 = score.astype(np.float32)
        nan = np.isnan(s32)
        want = np.lexsort((idx, np.where(nan, 0.0, -s32.astype(np.float64)), nan))
        k = min(n, 65536)
        assert np.array_equal(active.top_k(torch.from_numpy(s32).to(gpu), k).cpu().numpy(), want[:k])
    with pytest.raises(Exception, match="not excluded"):
        active.top_k(s_dev, remaining + 1, ex)


@pytest.mark.gpu
def test_top_k_launch_count_depends_on_the_sizes_only(gpu):
    """the same number of launches for a given (n, k) whatever the scores, and the used set does not add any"""
    from weasal_amd import _lib, active
    lib = _lib.lib()
    counts = []
    for seed, m in ((1, 0), (2, 0), (3, 50000)):
        rng = np.random.default_rng(seed)
        s = torch.from_numpy(rng.standard_normal(100000)).to(gpu)
        ex = rng.integers(0, 100000, size=m)
        before = lib.ws_launch_count()
        active.top_k(s, 3000, ex)
        counts.append(lib.ws_launch_count() - before)
    assert counts[0] == counts[1] == counts[2] and counts[0] > 0


# ------------------------------------------------------------------------------------------------------------------
# 3. point selection end to end
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("source,k,n_used", [("synthetic", 5000, 10000), ("g11", 200, 300)])
def test_select_points_against_the_restatement(gpu, syn, source, k, n_used):
    from weasal_amd import active
    probs = golden("g11_tester.npz")["test_probs"] if source == "g11" else syn
    n = probs.shape[0]
    rng = np.random.default_rng(17)
    used = rng.choice(n, size=n_used, replace=False).astype(np.int64)
    ref_score = active_ref.point_scores(probs, CLASS_W)[2]
    t = H_TOL * np.exp(CLASS_W).max()
    got = active.select_points(Votes([torch.from_numpy(probs).to(gpu)]), 0, CLASS_W, used, k)
    assert got.is_cuda
    assert_band_selection(ref_score, used, got.cpu().numpy(), k, t)


# ------------------------------------------------------------------------------------------------------------------
# 4. anchors
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_anchor_scores_and_selection(gpu, syn):
    from weasal_amd import active
    n_anchors, k = 3000, 200
    ptr, idx, labels = active_ref.synthetic_anchors(23, N_SYN, n_anchors, C9)
    sizes = np.diff(ptr)
    assert sizes.min() >= 50 and sizes.max() <= 4000 and labels.shape == (n_anchors, C9)
    used = np.random.default_rng(29).choice(n_anchors, size=400, replace=False).astype(np.int64)
    cs = active_ref.anchor_class_score(labels, used)
    ref = active_ref.anchor_scores(syn, ptr, idx, cs)
    dev = lambda a: torch.from_numpy(a).to(gpu)
    probs = dev(syn)
    h, p, _ = active.point_scores(probs, np.zeros(C9))
    got = active.anchor_scores(h, p, dev(ptr), dev(idx), cs)
    assert got.dtype == torch.float32 and got.shape == (n_anchors,)
    got = got.cpu().numpy()
    tol = H_TOL * cs.sum() + 32 * 2.0 ** -24 * np.abs(ref)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    print("anchors: max |got - ref| = %.3g, smallest slack %.3g" % (err.max(), (tol - err).min()))
    assert (err <= tol).all()
    # an empty anchor and one whose points were never voted on score 0
    ptr2 = np.array([0, 0, 3], np.int64)
    z = np.flatnonzero(syn.sum(1) == 0)[:3].astype(np.int64)
    assert active.anchor_scores(h, p, dev(ptr2), dev(z), cs).cpu().tolist() == [0.0, 0.0]
    # selection
    sel = active.select_anchors(Votes([probs]), 0, dev(ptr), dev(idx), labels, used, k)
    assert_band_selection(ref.astype(np.float64), used, sel.cpu().numpy(), k, float(tol.max()))


# ------------------------------------------------------------------------------------------------------------------
# 5. exhaustion
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_exhaustion_raises_the_reference_messages(gpu):
    from weasal_amd import active, tester
    probs = torch.from_numpy(active_ref.synthetic_votes(3, 1000, C9)).to(gpu)
    votes = Votes([probs])
    used = np.concatenate([np.arange(900), np.arange(100)])                    # 900 unique ids
    assert active.select_points(votes, 0, CLASS_W, used, 100).shape == (100,)
    with pytest.raises(ValueError, match='Not enough point labels left for the next iteration'):
        active.select_points(votes, 0, CLASS_W, used, 101)
    with pytest.raises(ValueError, match='Not enough point labels left for the next iteration'):
        tester.active_learning_selection(votes, CLASS_W, [used], 101)
    ptr, idx, labels = active_ref.synthetic_anchors(4, 1000, 20, C9, lo=5, hi=50)
    ptr_d, idx_d = torch.from_numpy(ptr).to(gpu), torch.from_numpy(idx).to(gpu)
    used_a = np.arange(15)
    assert active.select_anchors(votes, 0, ptr_d, idx_d, labels, used_a, 5).shape == (5,)
    with pytest.raises(ValueError, match='Not enough weak labels left for the next iteration'):
        active.select_anchors(votes, 0, ptr_d, idx_d, labels, used_a, 6)


# ------------------------------------------------------------------------------------------------------------------
# 6. reveal_labels
# ------------------------------------------------------------------------------------------------------------------
class SamplerCfg:
    in_features_dim = 3
    in_radius = 3.0
    augment_rotation = 'vertical'
    augment_scale_anisotropic = True
    augment_scale_min = 0.9
    augment_scale_max = 1.1
    augment_symmetries = [True, False, False]
    augment_noise = 0.0
    batch_num = 4


@pytest.mark.gpu
def test_reveal_labels_serves_the_truth_in_the_next_batch(gpu):
    from weasal_amd.sampler import SphereSampler, label_lut
    label_values = np.arange(1, 10)                                             # raw values 1..9 -> positions 0..8
    lut = label_lut(label_values)
    tiles = [sampler_ref.slab_cloud(41, 200000, 12.0, 1.0, 0.4), sampler_ref.slab_cloud(42, 90000, 9.0, 1.0, 0.4)]
    tiles = [(p, l + 1) for p, l in tiles]                                      # pseudo labels, raw values
    n0 = len(tiles[0][0])
    assert n0 > 10000
    rng = np.random.default_rng(6)
    truth = rng.integers(1, 10, size=n0).astype(np.int32)
    ids = rng.choice(n0, size=5000, replace=False).astype(np.int64)

    def make():
        return SphereSampler(SamplerCfg(), [(torch.from_numpy(p).to(gpu), torch.from_numpy(l).to(gpu)) for p, l in tiles],
                             label_values=label_values, seed=9, max_spheres=16, batch_limit=12000)
    plain, revealed = make(), make()
    ptr_before = revealed.sub_labels[0].data_ptr()
    revealed.reveal_labels(0, torch.from_numpy(ids).to(gpu), truth)
    assert revealed.sub_labels[0].data_ptr() == ptr_before                      # in place: the buffer the handle reads
    want = tiles[0][1].copy()
    want[ids] = truth[ids]
    assert np.array_equal(revealed.sub_labels[0].cpu().numpy(), want)
    assert np.array_equal(revealed.sub_labels[1].cpu().numpy(), tiles[1][1])
    is_revealed = np.zeros(n0, bool)
    is_revealed[ids] = True
    seen = 0
    for _ in range(3):
        a, b = plain.sample(), revealed.sample()
        for x, y in zip(a[:2] + a[4:], b[:2] + b[4:]):                          # everything but labels / lengths
            assert torch.equal(x, y)
        assert np.array_equal(a[3], b[3])
        la, lb = a[2].cpu().numpy(), b[2].cpu().numpy()
        cloud_of_row = np.repeat(b[6].cpu().numpy(), b[3])
        inds = b[8].cpu().numpy()
        hit = (cloud_of_row == 0) & is_revealed[np.where(cloud_of_row == 0, inds, 0)]
        assert np.array_equal(lb[hit], lut[truth[inds[hit]]])
        assert np.array_equal(lb[~hit], la[~hit])
        seen += int(hit.sum())
    assert seen > 100, "the batches were meant to contain revealed points"
    with pytest.raises(ValueError):
        revealed.reveal_labels(0, [n0], truth)
    with pytest.raises(ValueError):
        revealed.reveal_labels(0, [0], truth[:-1])


# ------------------------------------------------------------------------------------------------------------------
# 7. the tester's entry
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_active_learning_selection_appends_per_cloud(gpu):
    from weasal_amd import active, tester
    sizes = (40000, 25000)
    votes = tester.VoteAccumulator(sizes, C9, gpu)
    for i, n in enumerate(sizes):
        votes.probs[i].copy_(torch.from_numpy(active_ref.synthetic_votes(50 + i, n, C9)).to(gpu))
    rng = np.random.default_rng(8)
    used = [rng.choice(n, size=m, replace=False).astype(np.int64) for n, m in zip(sizes, (3000, 0))]
    k = 1500
    out = tester.active_learning_selection(votes, CLASS_W, used, k)
    assert len(out) == 2
    for i in range(2):
        assert isinstance(out[i], np.ndarray) and out[i].dtype == np.int64 and out[i].shape == (len(used[i]) + k,)
        assert np.array_equal(out[i][:len(used[i])], used[i])
        direct = active.select_points(votes, i, CLASS_W, used[i], k).cpu().numpy()
        assert np.array_equal(out[i][len(used[i]):], direct)
        assert len(np.unique(out[i])) == len(out[i])
    again = tester.active_learning_selection(votes, CLASS_W, out, k)           # the next iteration goes on from the lists
    for i in range(2):
        assert np.array_equal(again[i][:len(out[i])], out[i]) and len(np.unique(again[i])) == len(used[i]) + 2 * k
