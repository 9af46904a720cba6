"""GPU: pseudo-label refinement (weasal_amd.refine, csrc/refine.hip) against tests/refine_ref.py run on the CPU in the
same test.  Every step is exact -- a 0/1 product is an AND, the comparison is a float32 widened to float64 against the
host's double, counts are integers -- so every comparison here is equality; there is no tolerance.

Sizes: N = 1, 64 (one wave), 65, and 70 001 -- 274 tiles of 256 points, the last of one point, walked by workgroups that
take several tiles each, and more elements than one pass of the element-wise grid.  C = 1, 9 (36-byte rows) and 32 (bit 31).
"""
import numpy as np
import pytest
import torch

from conftest import golden

import active_ref
import refine_ref

NS = [1, 64, 65, 70001]
CS = [1, 9, 32]
THRESHOLDS = [0, 10, 20, 100]
N_COUNTS = [8, 9, 32]
PRED_VALUES = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 31, 40, -1], np.int32)     # below and above every n_counts, negative


def dev_u32(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32)).to(gpu)


# ------------------------------------------------------------------------------------------------------------------
# 1. the mask
# ------------------------------------------------------------------------------------------------------------------
def mask_case(n, c, seed):
    """index lists, label rows [A, c], the row that covers every point, and a selection that leaves it out"""
    rng = np.random.default_rng(seed)
    low = max(1, (6 * n) // 10)                              # the random anchors stay below 0.6 n
    lists = [[], [0], list(range(n)), [n - 1, n - 1, 0, n - 1], [2 % n, 3 % n], [1 % n], [1 % n, 2 % n], [1 % n], [],
             [max(n - 2, 0)]]
    for _ in range(12):
        lists.append(rng.integers(0, low, size=rng.integers(1, max(2, n // 8))).tolist())     # with repeats
    labels = (rng.random((len(lists), c)) < 0.7).astype(np.int64)
    labels[2] = 1
    labels[2, c // 2] = 0 if c > 1 else 1                    # the row over all N clears one class, not bit c - 1
    labels[4] = 0                                            # a label row without any class
    labels[5:8, c - 1] = (1, 0, 1)
    all_row = 2
    sel = np.array([9, 21, 7, 7, 4, 0, 5, 6, 9, 15, 3, 12, 11, 21, 1, 8], np.int64)   # repeats, not ascending, row 2 left out
    return lists, labels, all_row, sel


@pytest.mark.gpu
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("n", NS)
def test_weak_label_mask(gpu, n, c):
    from weasal_amd import refine
    lists, labels, all_row, sel = mask_case(n, c, 1000 + n % 101 + c)
    ptr, idx = refine_ref.csr(lists)
    assert len(lists[all_row]) == n and not labels[4].any() and (np.diff(ptr) == 0).any() and (np.diff(ptr) == 1).any()
    assert all_row not in sel and len(np.unique(sel)) < len(sel) and (np.diff(sel) < 0).any()
    if n >= 64:
        member = np.zeros(n, np.int64)
        for a in np.unique(sel):
            member[np.unique(np.asarray(lists[a], np.int64))] += 1
        assert (member == 0).any() and (member == 1).any() and (member >= 3).any()
    ptr_d, idx_d = torch.from_numpy(ptr).to(gpu), torch.from_numpy(idx).to(gpu)
    for use in (None, sel, torch.from_numpy(sel).to(gpu), np.zeros(0, np.int64)):
        host_use = use.cpu().numpy() if isinstance(use, torch.Tensor) else use
        want = refine_ref.mask_bits(refine_ref.weak_labels(n, ptr, idx, labels, host_use))
        got = refine.weak_label_mask(n, ptr_d, idx_d, labels, use)
        assert got.dtype == torch.uint32 and got.shape == (n,) and got.is_cuda and got.classes == c
        assert np.array_equal(got.cpu().numpy(), want), (n, c, None if use is None else len(use))
    if c == 32 and n > 1:
        full = refine_ref.mask_bits(refine_ref.weak_labels(n, ptr, idx, labels))
        assert (full >> 31 & 1).min() == 0 and (full >> 31 & 1).max() == 1          # bit 31 both cleared and kept


@pytest.mark.gpu
@pytest.mark.parametrize("n,c", [(65, 9), (70001, 32)])
def test_weak_label_mask_skips_and_reports_indices_out_of_range(gpu, n, c):
    from weasal_amd import refine
    lists, labels, _, sel = mask_case(n, c, 77 + c)
    ptr, idx = refine_ref.csr(lists)
    ptr_d = torch.from_numpy(ptr).to(gpu)
    bad_lists = [list(l) for l in lists]
    bad_lists[3].insert(1, n)                                 # one past the end
    bad_lists[12].insert(0, -1)
    bad_lists[2].insert(n // 2, 1 << 40)
    bad_ptr, bad_idx = refine_ref.csr(bad_lists)
    bad_sel = np.concatenate([sel[:5], [len(lists), -1], sel[5:]])
    want_all = refine_ref.mask_bits(refine_ref.weak_labels(n, ptr, idx, labels))
    want_sel = refine_ref.mask_bits(refine_ref.weak_labels(n, ptr, idx, labels, sel))
    # with the caller's status words nothing is read: the in-range part is the restatement without the bad entries
    st = refine.new_status(gpu)
    got = refine.weak_label_mask(n, torch.from_numpy(bad_ptr).to(gpu), torch.from_numpy(bad_idx).to(gpu), labels, None, st)
    assert np.array_equal(got.cpu().numpy(), want_all)
    assert st.cpu().tolist() == [3, 0, 0]
    with pytest.raises(ValueError, match="anchor_idx"):
        refine.raise_on_status(st.cpu().numpy())
    st = refine.new_status(gpu)
    got = refine.weak_label_mask(n, ptr_d, torch.from_numpy(idx).to(gpu), labels, bad_sel, st)
    assert np.array_equal(got.cpu().numpy(), want_sel)
    assert st.cpu().tolist() == [0, 2, 0]
    # without them the call reads its own and raises
    with pytest.raises(ValueError, match="anchor_idx"):
        refine.weak_label_mask(n, torch.from_numpy(bad_ptr).to(gpu), torch.from_numpy(bad_idx).to(gpu), labels)
    with pytest.raises(ValueError, match="use_anchors"):
        refine.weak_label_mask(n, ptr_d, torch.from_numpy(idx).to(gpu), labels, bad_sel)


# ------------------------------------------------------------------------------------------------------------------
# 2. refinement
# ------------------------------------------------------------------------------------------------------------------
def planted_values():
    """float32 votes next to the thresholds 20 % and 10 %: [at 0.2, below 0.2, above 0.01 * 10, below 0.01 * 10]"""
    thr10 = 0.01 * 10
    x = np.float32(thr10)
    lo, hi = (np.nextafter(x, np.float32(0)), x) if float(x) >= thr10 else (x, np.nextafter(x, np.float32(1)))
    assert float(lo) < thr10 <= float(hi) and np.nextafter(lo, np.float32(1)) == hi
    return np.array([np.float32(0.2), np.nextafter(np.float32(0.2), np.float32(0)), hi, lo], np.float32)


def refine_case(n, c, seed):
    """votes [m, c] with m = n + 5, predictions, the weak table of the points and a projection with repeats.  Rows 0..3
    hold the planted votes in column 0, which the weak labels of the points that read them allow (n >= 4); row 4 was
    never voted on."""
    rng = np.random.default_rng(seed)
    m = n + 5
    probs = active_ref.synthetic_votes(seed, m, c)
    preds = np.concatenate([np.full(4, 3), np.resize(PRED_VALUES[::-1], m - 4)]).astype(np.int32)
    weak = (rng.random((n, c)) < 0.6).astype(np.float64)
    weak[rng.random(n) < 0.05] = 0
    weak[rng.random(n) < 0.05] = 1
    proj = rng.integers(0, m, size=n).astype(np.int32)
    proj[n - n // 8:] = proj[n // 2] if n > 1 else 3          # an eighth of the points read one row
    probs[:5] = 0
    probs[:4, 0] = planted_values()
    if n >= 4:
        weak[:4, 0] = 1
        proj[:4] = np.arange(4)
    return m, probs, preds, weak, proj


@pytest.mark.gpu
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("n", NS)
def test_refine_labels(gpu, n, c):
    from weasal_amd import refine
    m, probs, preds, weak, proj = refine_case(n, c, 2000 + n % 103 + c)
    assert m != n and (probs.sum(1) == 0).any() and (n == 1 or (np.bincount(proj, minlength=m) > 1).any())
    assert not np.array_equal(proj, np.arange(n))
    assert (preds < 0).any() and (preds >= 32).any() and ((preds >= 0) & (preds < 8)).any()
    mask = dev_u32(refine_ref.mask_bits(weak), gpu)
    probs_d, preds_d, proj_d = torch.from_numpy(probs).to(gpu), torch.from_numpy(preds).to(gpu), torch.from_numpy(proj).to(gpu)
    if n >= 4:
        # the planted votes fall on both sides of the test, by the restatement alone
        for pj in (None, proj):
            p_, q_ = (probs[:n], preds[:n]) if pj is None else (probs, preds)
            at20 = refine_ref.refine(p_, q_, weak, 20, pj)[0][:4]
            at10 = refine_ref.refine(p_, q_, weak, 10, pj)[0][:4]
            assert at20.tolist() == [3, 10, 10, 10] and at10.tolist() == [3, 3, 3, 10]
    if n >= 64:
        # reading the weak labels through the projection too would give other labels: the test can tell
        weak_projected = np.concatenate([weak, np.ones((m - n, c))])[proj]
        assert not np.array_equal(refine_ref.refine(probs, preds, weak_projected, 10, proj)[0],
                                  refine_ref.refine(probs, preds, weak, 10, proj)[0])
    for pj, pj_d in ((None, None), (proj, proj_d)):
        p_, q_ = (probs[:n], preds[:n]) if pj is None else (probs, preds)
        p_d, q_d = (probs_d[:n], preds_d[:n]) if pj is None else (probs_d, preds_d)
        for thr in THRESHOLDS:
            for n_counts in N_COUNTS:
                want_l, want_c = refine_ref.refine(p_, q_, weak, thr, pj, n_counts)
                if thr == 0:
                    assert np.array_equal(want_l, q_ if pj is None else q_[pj])     # nothing emptied
                counts = torch.zeros(n_counts, dtype=torch.int64, device=gpu)
                got_l, got_c = refine.refine_labels(p_d, q_d, mask, thr, proj=pj_d, counts=counts)
                assert got_l.dtype == torch.int32 and got_l.shape == (n,) and got_c.data_ptr() == counts.data_ptr()
                assert np.array_equal(got_l.cpu().numpy(), want_l), (n, c, thr, n_counts, pj is not None)
                assert np.array_equal(got_c.cpu().numpy(), want_c), (n, c, thr, n_counts, pj is not None)
        # the counts accumulate: a second tile on the same buffer
        refine.refine_labels(p_d, q_d, mask, 10, proj=pj_d, counts=counts)
        assert np.array_equal(counts.cpu().numpy(), want_c + refine_ref.refine(p_, q_, weak, 10, pj, N_COUNTS[-1])[1])
    # the default buffer: one zeroed bin per class; another no_label
    got_l, got_c = refine.refine_labels(probs_d, preds_d, mask, 20, proj=proj_d, no_label=7)
    want_l, want_c = refine_ref.refine(probs, preds, weak, 20, proj, c, no_label=7)
    assert got_c.shape == (c,) and np.array_equal(got_l.cpu().numpy(), want_l) and np.array_equal(got_c.cpu().numpy(), want_c)


@pytest.mark.gpu
def test_refine_labels_counts_are_exact_when_every_point_predicts_one_class(gpu):
    from weasal_amd import refine
    n, c = 70001, 9
    _, probs, _, weak, _ = refine_case(n, c, 5)
    probs = probs[:n]
    preds = np.full(n, 5, np.int32)
    mask = dev_u32(refine_ref.mask_bits(weak), gpu)
    counts = torch.zeros(9, dtype=torch.int64, device=gpu)
    labels, _ = refine.refine_labels(torch.from_numpy(probs).to(gpu), torch.from_numpy(preds).to(gpu), mask, 0, counts=counts)
    assert counts.cpu().tolist() == [0, 0, 0, 0, 0, n, 0, 0, 0] and (labels == 5).all()
    want_l, want_c = refine_ref.refine(probs, preds, weak, 10, None, 9)
    assert 0 < want_c[5] < n and want_c.sum() == want_c[5]
    labels, _ = refine.refine_labels(torch.from_numpy(probs).to(gpu), torch.from_numpy(preds).to(gpu), mask, 10, counts=counts)
    assert np.array_equal(labels.cpu().numpy(), want_l)
    assert counts.cpu().tolist() == [0, 0, 0, 0, 0, n + int(want_c[5]), 0, 0, 0]


@pytest.mark.gpu
def test_refine_labels_skips_and_reports_a_projection_out_of_range(gpu):
    from weasal_amd import refine
    n, c = 70001, 9
    m, probs, preds, weak, proj = refine_case(n, c, 6)
    bad = np.array([5, 300, n - 1])
    proj = proj.copy()
    proj[bad] = (m, -1, np.iinfo(np.int32).max)
    ok = np.ones(n, bool)
    ok[bad] = False
    want_ok, want_c = refine_ref.refine(probs, preds, weak[ok], 10, proj[ok], 32)
    want_l = np.full(n, 10, np.int32)
    want_l[ok] = want_ok
    args = (torch.from_numpy(probs).to(gpu), torch.from_numpy(preds).to(gpu), dev_u32(refine_ref.mask_bits(weak), gpu), 10)
    st = refine.new_status(gpu)
    counts = torch.zeros(32, dtype=torch.int64, device=gpu)
    labels, _ = refine.refine_labels(*args, proj=torch.from_numpy(proj).to(gpu), counts=counts, status=st)
    assert np.array_equal(labels.cpu().numpy(), want_l)
    assert want_c[10] > 0 and np.array_equal(counts.cpu().numpy(), want_c)        # bin 10 holds the emptied points only
    assert st.cpu().tolist() == [0, 0, 3]
    with pytest.raises(ValueError, match="proj"):
        refine.read_counts(counts, st)
    with pytest.raises(ValueError, match="proj"):
        refine.refine_labels(*args, proj=torch.from_numpy(proj).to(gpu))
    assert np.array_equal(refine.read_counts(counts, refine.new_status(gpu)), want_c)


# ------------------------------------------------------------------------------------------------------------------
# 3. a tile end to end
# ------------------------------------------------------------------------------------------------------------------
def recorded_votes(probs, gpu):
    """a tester.VoteAccumulator filled from recorded votes"""
    from weasal_amd import tester
    votes = tester.VoteAccumulator([probs.shape[0]], probs.shape[1], gpu)
    votes.probs[0].copy_(torch.from_numpy(probs).to(gpu))
    return votes


def sphere_anchors(seed, probs, n_anchors=60, radius=0.9):
    """anchors drawn as spheres around random centres of synthetic coordinates; the label row of an anchor is the set of
    classes present in it (by a noisy arg-max 'truth'); plus overlap anchors that carry the product of two rows"""
    rng = np.random.default_rng(seed)
    n, c = probs.shape
    pts = rng.uniform(0, 6, size=(n, 3)).astype(np.float32)
    truth = np.argmax(probs, axis=1)
    flip = rng.random(n) < 0.2
    truth[flip] = rng.integers(0, c, size=int(flip.sum()))
    lists, rows = [], []
    for ctr in pts[rng.choice(n, size=n_anchors, replace=False)]:
        ids = np.flatnonzero(((pts - ctr) ** 2).sum(1) < radius * radius)
        lists.append(ids)
        rows.append(np.bincount(truth[ids], minlength=c) > 0)
    for a in range(4):                                       # each with the anchor it shares most points with
        shared = [len(np.intersect1d(lists[a], lists[j])) if j != a else -1 for j in range(n_anchors)]
        b = int(np.argmax(shared))
        lists.append(np.intersect1d(lists[a], lists[b]))
        rows.append(rows[a] & rows[b])
    return refine_ref.csr(lists) + (np.array(rows).astype(np.int64),)


@pytest.mark.gpu
def test_refine_cloud_against_the_restatement(gpu):
    from weasal_amd import refine
    probs = golden("g11_tester.npz")["test_probs"]
    n, c = probs.shape
    assert probs.dtype == np.float32 and c == 9
    ptr, idx, labels = sphere_anchors(31, probs)
    sizes = np.diff(ptr)
    covered = np.zeros(n, bool)
    covered[idx] = True
    assert sizes[-4:].min() > 0 and 0.1 < covered.mean() < 0.95 and 0 < labels.mean() < 1
    lv = np.arange(1, 10)                                     # label values 1..9: counts are by VALUE, bin 0 stays empty
    votes = recorded_votes(probs, gpu)
    ptr_d, idx_d = torch.from_numpy(ptr).to(gpu), torch.from_numpy(idx).to(gpu)
    use = np.random.default_rng(3).choice(len(sizes), size=40).astype(np.int64)
    for thr in (1, 3):                                        # per cent: these votes are young, the largest is 0.088
        for u in (None, use):
            want_l, want_c = refine_ref.refine_cloud(probs, lv, n, ptr, idx, labels, thr, u)
            got_l, got_c = refine.refine_cloud(votes, 0, ptr_d, idx_d, labels, thr, use_anchors=u, label_values=lv)
            assert got_l.dtype == torch.int32 and got_c.dtype == torch.int64 and got_c.shape == (c,)
            assert np.array_equal(got_l.cpu().numpy(), want_l) and np.array_equal(got_c.cpu().numpy(), want_c)
            assert want_c[0] == 0 and 0 < (want_l == 10).sum() < n
    # in place, into the tensor a sampler would keep as its resident label buffer; counts and status collected, one read
    out = torch.full((n,), -7, dtype=torch.int32, device=gpu)
    counts = torch.zeros(11, dtype=torch.int64, device=gpu)
    st = refine.new_status(gpu)
    got_l, got_c = refine.refine_cloud(votes, 0, ptr_d, idx_d, labels, 3, label_values=lv, counts=counts, out=out, status=st)
    assert got_l is out and got_l.data_ptr() == out.data_ptr() and got_c.data_ptr() == counts.data_ptr()
    want_l, want_c = refine_ref.refine_cloud(probs, lv, n, ptr, idx, labels, 3, n_counts=11)
    assert np.array_equal(out.cpu().numpy(), want_l)
    assert np.array_equal(refine.read_counts(counts, st), want_c) and want_c[10] == (want_l == 10).sum()
    with pytest.raises(ValueError, match="columns of the votes"):
        refine.refine_cloud(votes, 0, ptr_d, idx_d, labels[:, :8], 20)


# ------------------------------------------------------------------------------------------------------------------
# 4. the detour through the full-resolution cloud
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_roundtrip_projection_against_brute_force(gpu):
    from weasal_amd import ops, refine
    dl = 0.4
    full = np.random.default_rng(0).uniform(0, 4, size=(3000, 3)).astype(np.float32) + np.float32(100.0)
    full_d = torch.from_numpy(full).to(gpu)
    sub_d = ops.grid_subsample(full_d, [len(full)], dl)[0]
    sub = sub_d.cpu().numpy()
    assert 500 < len(sub) < 2000
    f0, s0 = full - full.min(0), sub - sub.min(0)             # each cloud reduced by its own minimum
    to_full, ties_a = refine_ref.nearest_brute(s0, f0)
    back, ties_b = refine_ref.nearest_brute(f0, s0)
    assert not ties_a.any() and not ties_b.any(), "the fixture has tied nearest distances: choose another seed"
    want = back[to_full]
    assert (want != np.arange(len(sub))).any(), "the composite is the identity: the fixture says nothing"
    got = refine.roundtrip_projection(full_d, sub_d, dl)
    assert got.dtype == torch.int32 and got.shape == (len(sub),)
    assert np.array_equal(got.cpu().numpy(), want)
