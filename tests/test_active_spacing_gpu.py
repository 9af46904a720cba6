"""GPU: the selection with a minimum spacing (active.spaced_top_k, ws_al_spaced_select) against the numpy restatement of
tests/active_spacing_ref.py.  Every comparison is torch.equal: the scores handed to both sides are the same float64
numbers, the distances are float64 on both sides with every operation rounded on its own, so there is no tolerance.

Every row (the table in tests/test_active_spacing_cpu.py) runs three times: twice through the C entry into fresh buffers
-- the ids between guard words that hold a sentinel, the scratch filled with 0xFF bytes with 256 guard bytes behind it, the
state words preset to garbage -- and once through active.spaced_top_k; the three results are equal to each other and to
the restatement."""
import ctypes as C

import numpy as np
import pytest
import torch

import active_ref
import active_spacing_ref as R

ROWS = R.rows()
SENTINEL = -0x0123456789ABCDEF
GUARD = 8              # int64 words in front of and behind the ids
CLASS_W = np.array([0.2, 1.0, 0.4, 1.8, 0.6, 1.4, 0.8, 1.2, 1.6])


class Votes:
    def __init__(self, probs):
        self.probs = probs


@pytest.fixture(scope="module")
def want():
    """the restatement of every row, computed once"""
    return {name: R.select(r["score"], r["coords"], r["used"], r["k"], r["spacing"]) for name, r in ROWS.items()}


def run_raw(gpu, score, coords, used, k, spacing, prefix=None):
    """the loop of active.spaced_top_k on guarded buffers -> (ids device int64 [k], accepted, runs)"""
    from weasal_amd import _lib, active
    lib = _lib.lib()
    n = score.shape[0]
    used = np.ascontiguousarray(used, np.int64)
    free = n - len(np.unique(used))
    run = prefix or max(active.SPACED_PREFIX_FACTOR * k, active.SPACED_PREFIX_MIN)
    box = torch.full((GUARD + k + GUARD,), SENTINEL, dtype=torch.int64, device=gpu)
    ids = box[GUARD:GUARD + k]
    state = torch.full((2,), -77, dtype=torch.int64, device=gpu)
    accepted = consumed = runs = 0
    while accepted < k and consumed < free:
        upto = min(free, consumed + run)
        cand = active.top_k(score, upto, used)[consumed:]
        m = upto - consumed
        nbytes = lib.ws_al_spaced_scratch_bytes(m, len(used), k)
        scratch = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device=gpu)
        rc = lib.ws_al_spaced_select(_lib.ptr(coords), int(coords.dtype == torch.float64), n, _lib.ptr(cand), m,
                                     C.c_void_p(used.ctypes.data), len(used), float(spacing), k, _lib.ptr(ids), _lib.ptr(state),
                                     int(runs > 0), _lib.ptr(scratch), _lib.current_stream())
        assert rc == 0, lib.ws_last_error()
        accepted, seen = state.cpu().tolist()
        assert (scratch[nbytes:] == 0xFF).all(), "the scratch guard was written"
        consumed, runs, run = upto, runs + 1, run * active.SPACED_PREFIX_GROWTH
        assert seen <= consumed and (accepted == k or seen == consumed)
    assert (box[:GUARD] == SENTINEL).all() and (box[GUARD + k:] == SENTINEL).all(), "the ids guard was written"
    assert (ids[accepted:] == SENTINEL).all(), "ids beyond the acceptances were written"
    return ids.clone(), accepted, runs


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ROWS))
def test_rows_equal_the_restatement(gpu, want, name):
    from weasal_amd import active
    r = ROWS[name]
    score = torch.from_numpy(r["score"]).to(gpu)
    coords = torch.from_numpy(r["coords"]).to(gpu)
    ref = torch.from_numpy(want[name])
    first = run_raw(gpu, score, coords, r["used"], r["k"], r["spacing"], r["prefix"])
    second = run_raw(gpu, score, coords, r["used"], r["k"], r["spacing"], r["prefix"])
    assert first[1] == second[1] == r["k"] and first[2] == second[2]
    assert torch.equal(first[0], second[0]), "two runs differ"
    assert torch.equal(first[0].cpu(), ref)
    got = active.spaced_top_k(score, coords, r["k"], r["spacing"], r["used"], prefix=r["prefix"])
    assert got.dtype == torch.int64 and got.is_cuda and torch.equal(got.cpu(), ref)
    assert active.last_spaced["passes"] == first[2]
    print("row %s: %d runs, %d candidates handed over for k = %d" % (name, first[2], active.last_spaced["consumed"], r["k"]))
    if name == 'f':
        assert first[2] > 1, "row f must resume"
    elif r["prefix"] is None:
        assert first[2] == 1, "the default prefix was meant to make one run the normal case"
    if name == 'b_0.5':
        assert sorted(got.cpu().tolist()) == list(range(512))
    if name == 'c':
        assert (np.diff(want[name]) > 0).all()                   # all scores equal: the order falls to the ids
    # host coordinates (the anchors' centres live there) and device id lists are accepted too
    again = active.spaced_top_k(score, r["coords"], r["k"], r["spacing"], torch.from_numpy(r["used"]).to(gpu), prefix=r["prefix"])
    assert torch.equal(again.cpu(), ref)


@pytest.mark.gpu
def test_exhaustion_and_empty_requests(gpu):
    """row h: n_used = 0; k = 0; k = the number of acceptable points exactly; one more"""
    from weasal_amd import _lib, active
    lib = _lib.lib()
    h = ROWS['h']
    score, coords = torch.from_numpy(h["score"]).to(gpu), torch.from_numpy(h["coords"]).to(gpu)
    most = R.acceptable(h["score"], h["coords"], h["used"], h["spacing"])
    before = lib.ws_launch_count()
    none = active.spaced_top_k(score, coords, 0, h["spacing"])
    assert none.shape == (0,) and none.dtype == torch.int64 and lib.ws_launch_count() == before
    got, accepted, runs = run_raw(gpu, score, coords, h["used"], most, h["spacing"])
    assert accepted == most and runs == 1
    assert torch.equal(got.cpu(), torch.from_numpy(R.select(h["score"], h["coords"], h["used"], most, h["spacing"])))
    assert torch.equal(active.spaced_top_k(score, coords, most, h["spacing"]), got)
    part, accepted, runs = run_raw(gpu, score, coords, h["used"], most + 1, h["spacing"])
    assert accepted == most and torch.equal(part[:most], got) and part[most].item() == SENTINEL
    with pytest.raises(ValueError, match='Not enough point labels left for the next iteration .*min_spacing 1.5'):
        active.spaced_top_k(score, coords, most + 1, h["spacing"], exhausted=R.POINT_MESSAGE)
    with pytest.raises(ValueError, match='Not enough point labels left for the next iteration'):
        active.select_points(Votes([torch.from_numpy(active_ref.synthetic_votes(3, 200, 9)).to(gpu)]), 0, CLASS_W, [], 150,
                             points=coords, min_spacing=h["spacing"])
    # an empty run of candidates: nothing launched, a fresh walk's state zeroed
    state = torch.full((2,), 5, dtype=torch.int64, device=gpu)
    before = lib.ws_launch_count()
    assert lib.ws_al_spaced_select(_lib.ptr(coords), 0, 200, None, 0, None, 0, 1.0, 4, None, _lib.ptr(state), 0, None,
                                   _lib.current_stream()) == 0
    assert lib.ws_launch_count() == before and state.cpu().tolist() == [0, 0]
    with pytest.raises(ValueError, match="excluded ids"):
        active.spaced_top_k(score, coords, 2, 1.0, [200])
    with pytest.raises(ValueError, match=r"coordinates must be \[200, 3\]"):
        active.spaced_top_k(score, coords[:100], 2, 1.0)
    with pytest.raises(_lib.WeasalHipError, match="WS_AL_SPACED_MAX_K"):
        active.spaced_top_k(torch.zeros(8000, dtype=torch.float64, device=gpu), torch.zeros(8000, 3, device=gpu),
                            _lib.ABI.constants["WS_AL_SPACED_MAX_K"] + 1, 1.0)


@pytest.mark.gpu
def test_anchor_selection_with_float64_centres(gpu):
    """row g through active.select_anchors, the restatement fed the anchor scores the device computed"""
    from weasal_amd import active
    g = ROWS['g']
    centres, used, k, s = g["coords"], g["used"], g["k"], g["spacing"]
    assert centres.dtype == np.float64
    n_points = 3000
    probs = torch.from_numpy(active_ref.synthetic_votes(31, n_points, 9)).to(gpu)
    a_ptr, a_idx, labels = R.lattice_anchors(32, n_points, centres)
    d_ptr, d_idx = torch.from_numpy(a_ptr).to(gpu), torch.from_numpy(a_idx).to(gpu)
    entropy, preds, _ = active.point_scores(probs, np.zeros(9))
    score = active.anchor_scores(entropy, preds, d_ptr, d_idx, active_ref.anchor_class_score(labels, used))
    score64 = score.cpu().numpy().astype(np.float64)
    ref = R.select(score64, centres, used, k, s, R.ANCHOR_MESSAGE)
    plain = active.select_anchors(Votes([probs]), 0, d_ptr, d_idx, labels, used, k)
    assert np.array_equal(plain.cpu().numpy(), active_ref.select(score64, used, k))
    assert not np.array_equal(plain.cpu().numpy(), ref), "the spacing was meant to change this selection"
    got = active.select_anchors(Votes([probs]), 0, d_ptr, d_idx, labels, used, k, centres=centres, min_spacing=s)
    assert torch.equal(got.cpu(), torch.from_numpy(ref))
    most = R.acceptable(score64, centres, used, s)
    with pytest.raises(ValueError, match='Not enough weak labels left for the next iteration'):
        active.select_anchors(Votes([probs]), 0, d_ptr, d_idx, labels, used, most + 1, centres=centres, min_spacing=s)


@pytest.mark.gpu
def test_no_spacing_is_the_plain_selection_launch_for_launch(gpu):
    from weasal_amd import _lib, active, tester
    lib = _lib.lib()
    n, k = 20000, 300
    probs = torch.from_numpy(active_ref.synthetic_votes(41, n, 9)).to(gpu)
    votes = Votes([probs])
    pts = torch.rand(n, 3, device=gpu)
    used = np.random.default_rng(3).choice(n, size=500, replace=False).astype(np.int64)

    def counted(fn):
        before = lib.ws_launch_count()
        out = fn()
        return out, lib.ws_launch_count() - before
    _, _, score = active.point_scores(probs, CLASS_W)
    plain, n_plain = counted(lambda: active.top_k(score, k, used))
    base, n_base = counted(lambda: active.select_points(votes, 0, CLASS_W, used, k))
    assert torch.equal(base, plain) and n_base == n_plain + 1                          # the score kernel
    for spacing in (0.0, None, 0):
        got, launches = counted(lambda: active.select_points(votes, 0, CLASS_W, used, k, points=pts, min_spacing=spacing))
        assert torch.equal(got, plain) and launches == n_base
        got, launches = counted(lambda: active.spaced_top_k(score, pts, k, spacing, used))
        assert torch.equal(got, plain) and launches == n_plain
        out, launches = counted(lambda: tester.active_learning_selection(votes, CLASS_W, [used], k, points=[pts], min_spacing=spacing))
        assert np.array_equal(out[0], np.append(used, plain.cpu().numpy())) and launches == n_base
    out, launches = counted(lambda: tester.active_learning_selection(votes, CLASS_W, [used], k))
    assert np.array_equal(out[0], np.append(used, plain.cpu().numpy())) and launches == n_base


@pytest.mark.gpu
def test_active_learning_selection_with_a_spacing(gpu):
    """two clouds, the appended lists against the restatement fed the device's scores"""
    from weasal_amd import active, tester
    rng = np.random.default_rng(9)
    sizes, k, s = (6000, 2500), 40, 3.0
    probs = [torch.from_numpy(active_ref.synthetic_votes(60 + i, n, 9)).to(gpu) for i, n in enumerate(sizes)]
    pts = [rng.uniform([0, 0, 0], [40, 40, 4], size=(n, 3)).astype(np.float32) for n in sizes]
    used = [rng.choice(sizes[0], size=200, replace=False).astype(np.int64), np.zeros(0, np.int64)]
    votes = Votes(probs)
    out = tester.active_learning_selection(votes, CLASS_W, used, k, points=[torch.from_numpy(p).to(gpu) for p in pts], min_spacing=s)
    assert len(out) == 2
    for i in range(2):
        score = active.point_scores(probs[i], CLASS_W)[2].cpu().numpy()
        ref = R.select(score, pts[i], used[i], k, s)
        assert out[i].dtype == np.int64 and np.array_equal(out[i], np.append(used[i], ref))
        assert not np.array_equal(ref, active_ref.select(score, used[i], k))
