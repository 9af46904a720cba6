"""CPU (no GPU needed): the selection with a minimum spacing.  The numpy restatement (tests/active_spacing_ref.py) is held
to the properties that define it, by code that shares nothing with it (a full pairwise distance matrix); every wrong
variant is shown to differ from it on some row; the argument checks of the library's entries, which happen before the
device is touched; the reporter's text for the row that reaches each kernel path; `al_min_spacing` in parameters.txt; and
what the two testers hand to the selection.

Rows (active_spacing_ref.rows(); the GPU test runs the same ones):
  a       5000 points in a 50 x 50 x 5 box, a smooth score quantised to 64 levels, 100 used ids, k = 64, s = 2
  b_0.5   an 8 x 8 x 8 lattice of pitch 0.5 with s = 0.5: a neighbour at exactly s is not blocked, all 512 are acceptable
  b_0.75  the same lattice with s = 0.75
  c       (a) with all scores equal        d  (a) with 10 % NaN scores and a top level of mixed -0.0 / +0.0
  e       3000 points on a line 0.3 apart, decreasing scores, s = 0.5, k = 300; e_long: k = 1500, every chunk of the walk
  f       10000 points whose 6000 best lie within s / 2 of one point, prefix 256, k = 32
  g       float64 centres: a lattice and the centres half way between x-neighbours, 6 used
  h       200 points, for the exhaustion cases
  t       pairs at a distance that float32 arithmetic decides differently from float64
"""
import ctypes as C
import os

import numpy as np
import pytest

import active_ref
import active_spacing_ref as R

ROWS = R.rows()
BITES = ('a', 'e', 'f')


def pairwise_d2(a, b):
    """float64 [len(a), len(b)], one axis at a time"""
    a, b = np.asarray(a).astype(np.float64), np.asarray(b).astype(np.float64)
    dx, dy, dz = (a[:, None, i] - b[None, :, i] for i in range(3))
    return (dx * dx + dy * dy) + dz * dz


@pytest.fixture(scope="module")
def walks():
    return {name: R.walk(r["score"], r["coords"], r["used"], r["k"], r["spacing"]) for name, r in ROWS.items()}


@pytest.mark.parametrize("name", sorted(ROWS))
def test_restatement_properties(walks, name):
    r = ROWS[name]
    ids, behind = walks[name]
    s2 = np.float64(r["spacing"]) * np.float64(r["spacing"])
    used = np.unique(r["used"])
    assert ids.shape == (r["k"],) and len(np.unique(ids)) == r["k"] and not np.isin(ids, used).any()
    cand = active_ref.select(r["score"], r["used"], len(r["score"]) - len(used))      # the plain order, used removed
    assert np.array_equal(cand[np.isin(cand, ids)], ids), "acceptance order is the priority order"
    assert cand[behind - 1] == ids[-1]
    front = cand[:behind]
    sel = np.flatnonzero(np.isin(front, ids))                                         # positions of the accepted ones
    k = len(sel)
    d2 = pairwise_d2(r["coords"][front], r["coords"][np.concatenate([ids, used])])   # [front, accepted + used]
    pair = d2[sel, :k]
    assert (pair[~np.eye(k, dtype=bool)] >= s2).all(), "two selected ids closer than the spacing"
    assert (d2[sel, k:] >= s2).all(), "a selected id closer than the spacing to a used one"
    near = d2 < s2
    near[:, :k] &= sel[None, :] < np.arange(behind)[:, None]                          # only what was accepted earlier blocks
    skipped = ~np.isin(front, ids)
    free = np.flatnonzero(skipped & ~near.any(axis=1))
    assert len(free) == 0, "candidates %s were skipped though nothing blocks them" % front[free][:5]


def test_every_wrong_variant_differs_on_some_row(walks):
    for wrong, _ in R.WRONG:
        differs = []
        for name, r in ROWS.items():
            got = R.wrong(wrong, r["score"], r["coords"], r["used"], r["k"], r["spacing"])
            if not (isinstance(got, np.ndarray) and np.array_equal(got, walks[name][0])):
                differs.append(name)
        print("%-48s differs on %s" % (wrong, ", ".join(differs)))
        assert differs, "no row tells '%s' from the contract" % wrong


@pytest.mark.parametrize("name", BITES)
def test_the_spacing_bites(walks, name):
    ids, behind = walks[name]
    in_front = behind - 1
    blocked = in_front - (len(ids) - 1)
    share = blocked / in_front
    assert share >= 0.5, "row %s: %d of the %d candidates in front of the last acceptance are blocked (%.1f %%)" % (
        name, blocked, in_front, 100 * share)


def test_lattice_at_exactly_the_spacing_and_exhaustion():
    b = ROWS['b_0.5']
    assert R.acceptable(b["score"], b["coords"], b["used"], b["spacing"]) == 512
    h = ROWS['h']
    most = R.acceptable(h["score"], h["coords"], h["used"], h["spacing"])
    assert 8 < most < 200
    assert len(R.select(h["score"], h["coords"], h["used"], most, h["spacing"])) == most
    with pytest.raises(ValueError, match='Not enough point labels left for the next iteration .*1.5'):
        R.select(h["score"], h["coords"], h["used"], most + 1, h["spacing"])
    with pytest.raises(ValueError, match='Not enough weak labels left for the next iteration'):
        R.select(h["score"], h["coords"], h["used"], most + 1, h["spacing"], R.ANCHOR_MESSAGE)


# ------------------------------------------------------------------------------------------------------------------
# the library, before the device is touched
# ------------------------------------------------------------------------------------------------------------------
def _host(a):
    return C.c_void_p(a.ctypes.data)


def test_spaced_entries_validate_before_touching_the_device():
    from weasal_amd import _lib
    lib = _lib.lib()
    cap = _lib.ABI.constants["WS_AL_SPACED_MAX_K"]
    assert cap >= 4096
    null, one = C.c_void_p(None), C.c_void_p(16)                  # `one` is never dereferenced: validation fails first
    used = np.array([1, 1, 2], np.int64)

    def call(n=10, m=5, h_used=null, n_used=0, spacing=1.0, k=2, coords=one, cand=one, ids=one, state=one, scratch=one, f64=0):
        return lib.ws_al_spaced_select(coords, f64, n, cand, m, h_used, n_used, spacing, k, ids, state, 0, scratch, null)
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(spacing=bad) == 1 and b"spacing" in lib.ws_last_error()
    assert call(k=-1) == 1
    assert call(m=-1) == 1 and call(n=-1) == 1 and call(n_used=-1) == 1
    assert call(k=cap + 1) == 2 and b"WS_AL_SPACED_MAX_K" in lib.ws_last_error()
    for bad in (10, -1, 1 << 40):
        ex = np.array([3, bad], np.int64)
        assert call(h_used=_host(ex), n_used=2) == 1 and b"outside [0, 10)" in lib.ws_last_error()
    assert call(h_used=null, n_used=3) == 1 and b"NULL" in lib.ws_last_error()
    for missing in ("coords", "cand", "ids", "state", "scratch"):
        assert call(h_used=_host(used), n_used=3, **{missing: null}) == 1 and b"NULL" in lib.ws_last_error()
    # nothing asked for: no pointer is needed and nothing is launched (a NULL state is not zeroed either)
    assert call(k=0, coords=null, cand=null, ids=null, state=null, scratch=null) == 0
    assert call(m=0, coords=null, cand=null, ids=null, state=null, scratch=null, h_used=_host(used), n_used=3) == 0
    # the scratch holds the used ids and a flag per candidate, whatever k
    sizes = [lib.ws_al_spaced_scratch_bytes(m, u, 64) for m, u in ((0, 0), (1000, 0), (1000, 500), (100000, 500))]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[2] >= 1000 + 500 * 8
    assert all(s % 256 == 0 for s in sizes)


def test_reporter_names_the_path_of_every_row():
    """the first run of every row as active.spaced_top_k hands it over, and the further runs of row f"""
    from weasal_amd import _lib, active
    lib = _lib.lib()

    def variant(r, m, resume=0):
        text = C.create_string_buffer(256)
        rc = lib.ws_al_spaced_variant(int(r["coords"].dtype == np.float64), len(r["score"]), m, len(r["used"]), r["spacing"],
                                      r["k"], resume, text, 256)
        assert rc == 0, lib.ws_last_error()
        return text.value.decode()

    def first_run(r):
        free = len(r["score"]) - len(np.unique(r["used"]))
        run = r["prefix"] or max(active.SPACED_PREFIX_FACTOR * r["k"], active.SPACED_PREFIX_MIN)
        return min(free, run)
    got = {name: variant(r, first_run(r)) for name, r in ROWS.items()}
    for name, text in got.items():
        print("%-7s %s" % (name, text))
    assert got['a'] == "spaced_used_kernel<float> blocks=16 tiles=1 + spaced_walk_kernel<float> chunks=4 tail=0 resume=0"
    assert got['b_0.5'] == "no used pass + spaced_walk_kernel<float> chunks=1 tail=512 resume=0"
    assert got['e_long'] == "no used pass + spaced_walk_kernel<float> chunks=3 tail=952 resume=0"
    assert len(np.unique(ROWS['g']["used"])) == 5                 # six used ids, one of them twice
    assert got['g'] == "spaced_used_kernel<double> blocks=1 tiles=1 + spaced_walk_kernel<double> chunks=1 tail=127 resume=0"
    f = ROWS['f']
    assert got['f'] == "no used pass + spaced_walk_kernel<float> chunks=1 tail=256 resume=0"
    assert variant(f, 1024, 1) == "no used pass + spaced_walk_kernel<float> chunks=1 tail=0 resume=1"
    assert variant(f, 10000 - 256 - 1024 - 4096, 1) == "no used pass + spaced_walk_kernel<float> chunks=5 tail=528 resume=1"
    text = C.create_string_buffer(64)
    assert lib.ws_al_spaced_variant(0, 10, 0, 0, 1.0, 5, 0, text, 64) == 0 and text.value == b"none (m == 0) state zeroed"
    assert lib.ws_al_spaced_variant(0, 10, 5, 0, 1.0, 0, 1, text, 64) == 0 and text.value == b"none (k == 0)"
    assert lib.ws_al_spaced_variant(0, 10, 5, 0, -1.0, 5, 0, text, 64) == 1
    assert lib.ws_al_spaced_variant(0, 10, 5, 0, 1.0, 5, 0, None, 64) == 1


def test_python_entries_check_the_spacing_on_the_host():
    import torch
    from weasal_amd import _lib, active, tester
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min_spacing"):
            active.spaced_top_k(torch.zeros(8, dtype=torch.float64), torch.zeros(8, 3), 2, bad)
        with pytest.raises(ValueError, match="min_spacing"):
            active.select_anchors(None, 0, None, None, None, [0], 1, centres=np.zeros((1, 3)), min_spacing=bad)

    class Votes:
        probs = [torch.zeros(8, 3)]
    with pytest.raises(ValueError, match="min_spacing"):
        tester.active_learning_selection(Votes(), [0, 0, 0], [[]], 2, points=[np.zeros((8, 3), np.float32)], min_spacing=-2.0)
    with pytest.raises(ValueError, match="one coordinate array per cloud"):
        tester.active_learning_selection(Votes(), [0, 0, 0], [[]], 2, min_spacing=1.0)
    with pytest.raises(_lib.WeasalHipError):                      # a spacing changes nothing about where the votes live
        active.spaced_top_k(torch.zeros(8, dtype=torch.float64), torch.zeros(8, 3), 2, 1.0)
    assert active._spacing(None) == 0.0 and active._spacing(0) == 0.0 and active._spacing(2.5) == 2.5


# ------------------------------------------------------------------------------------------------------------------
# parameters.txt
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dales_pl", "vaihingen3d_wl"])
def test_parameters_txt_without_the_key_is_unchanged_and_the_key_round_trips(name, tmp_path):
    from conftest import GOLDEN
    from weasal_amd.config import Config
    d = os.path.join(GOLDEN, "params", name)
    text = open(os.path.join(d, "parameters.txt"), "rb").read()
    cfg = Config().load(d)
    assert not hasattr(cfg, "al_min_spacing")
    cfg.saving_path = str(tmp_path)
    cfg.save()
    assert (tmp_path / "parameters.txt").read_bytes() == text
    cfg.al_min_spacing = 2.5
    (tmp_path / "spaced").mkdir()
    cfg.saving_path = str(tmp_path / "spaced")
    cfg.save()
    spaced = (tmp_path / "spaced" / "parameters.txt").read_bytes()
    assert spaced == text + b"al_min_spacing = 2.500000\n"
    back = Config().load(str(tmp_path / "spaced"))
    assert back.al_min_spacing == 2.5 and isinstance(back.al_min_spacing, float)
    (tmp_path / "again").mkdir()
    back.saving_path = str(tmp_path / "again")
    back.save()
    assert (tmp_path / "again" / "parameters.txt").read_bytes() == spaced


def test_no_configuration_class_declares_the_key():
    from weasal_amd import config as wcfg
    for cls in vars(wcfg).values():
        if isinstance(cls, type) and issubclass(cls, wcfg.Config):
            assert not hasattr(cls, "al_min_spacing") and not hasattr(cls(), "al_min_spacing")


# ------------------------------------------------------------------------------------------------------------------
# what the testers hand to the selection
# ------------------------------------------------------------------------------------------------------------------
class _Cfg:
    class_w = [1.0, 2.0, 3.0]
    added_labels_per_epoch = 7


class _Anchors:
    def __init__(self, tag):
        self.ptr, self.idx, self.lb, self.centres = "ptr" + tag, "idx" + tag, np.eye(3, dtype=np.int64), "centres" + tag


class _Votes:
    probs = [None, None]


@pytest.mark.parametrize("spacing", [None, 0.0, 2.5])
def test_select_of_both_testers_passes_the_configured_spacing(monkeypatch, spacing):
    import torch
    from weasal_amd import active, tester, testrun
    cfg = _Cfg()
    if spacing is not None:
        cfg.al_min_spacing = spacing
    calls = []
    monkeypatch.setattr(tester, "active_learning_selection", lambda *a, **kw: calls.append((a, kw)) or "points")
    monkeypatch.setattr(active, "select_anchors", lambda *a, **kw: calls.append((a, kw)) or torch.tensor([5], dtype=torch.int64))
    tiles = ["tile0", "tile1"]
    used = [np.array([1]), np.array([2])]
    t = object.__new__(testrun.ModelTester)
    t.config, t.votes = cfg, _Votes()
    assert t._select(None, sub_points=tiles, used_ids=used) == "points"
    (a, kw), = calls
    assert a == (t.votes, cfg.class_w, used, 7)
    assert kw == (dict(points=tiles, min_spacing=2.5) if spacing else {})
    del calls[:]
    w = object.__new__(testrun.ModelTesterWL)
    w.config, w.votes = cfg, _Votes()
    sets = [_Anchors("0"), _Anchors("1")]
    out = w._select(None, sub_points=tiles, anchor_sets=sets, used_anchors=used, added_labels=3)
    assert [o.tolist() for o in out] == [[1, 5], [2, 5]]
    assert len(calls) == 2
    for i, (a, kw) in enumerate(calls):
        assert a[:4] == (w.votes, i, "ptr%d" % i, "idx%d" % i) and a[5] is used[i] and a[6] == 3
        assert kw == (dict(centres="centres%d" % i, min_spacing=2.5) if spacing else {})
