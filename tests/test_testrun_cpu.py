"""CPU: the numpy restatement of the test run (tests/testrun_ref.py) against tests/golden/g21_test_run.npz -- the reference's
own `cloud_segmentation_test` of utils/tester_PseudoLabel.py (case A) and utils/tester_WeakLabel.py (case B), recorded by
tests/golden/make_golden_test_run.py --, the checkpoint rule on hand-written minima, and the argument checks of
ws_test_outputs, which are made before the device is touched."""
import hashlib
import os

import numpy as np
import pytest
import torch

import testrun_ref as ref
from conftest import GOLDEN, golden


@pytest.fixture(scope="module")
def g21():
    return golden("g21_test_run.npz")


def _case(g, tag):
    n = len(g[tag + "/cloud_sizes"])
    lv, ign = g[tag + "/label_values"], g[tag + "/ignored"]
    get = lambda name: [g["%s/%s_%d" % (tag, name, i)] for i in range(n)]
    return n, lv, ign, get


# ---------------------------------------------------------------------------------------------------------------------
# the checkpoint rule
# ---------------------------------------------------------------------------------------------------------------------
RULE_CASES = [
    # minima, num_votes, [(checkpoint, reproject)], ended
    ([0.3, 0.7, 1.2, 1.8], 1, [(False, False), (True, False), (False, False), (True, True)], True),      # the fixture's script
    ([0.6], 0, [(True, True)], True),                                                                    # 0.5 > 0 at once
    ([0.5, 0.5001], 0, [(False, False), (True, True)], True),                                            # strict <
    ([0.2, 0.4], 0, [(False, False), (False, False)], False),
    # a jump of more than one vote in an epoch: last_min still advances by one per epoch (-0.5 -> 0.5 -> 1.5 -> 2.5)
    ([3.7, 3.7, 3.7], 2, [(True, False), (True, False), (True, True)], True),
    ([3.7, 3.8], 1, [(True, False), (True, True)], True),
    ([0.9, 1.4, 1.6, 2.6], 1, [(True, False), (False, False), (True, True)], True),                      # ends before the last
    ([5.0], -1, [(True, True)], True),
]


@pytest.mark.parametrize("minima,num_votes,want,ended", RULE_CASES)
def test_checkpoint_rule_on_hand_written_minima(minima, num_votes, want, ended):
    from weasal_amd import testrun
    steps, done = ref.run_rule(minima, num_votes)
    assert [(c, r) for _, c, r in steps] == want and done == ended
    # the product's rule, epoch by epoch
    last_min, got = -0.5, []
    for new_min in minima:
        last_min, fired, end = testrun.checkpoint_rule(last_min, new_min, num_votes)
        got.append((fired, fired and end))
        if end:
            break
    assert got == want and end == ended


def test_rule_constants():
    from weasal_amd import testrun
    assert testrun.ModelTester.test_smooth == 0.95 and testrun.ModelTester.test_radius_ratio == 0.7
    assert testrun.ModelTester.results == 'test/PseudoLabel' and testrun.ModelTesterWL.results == 'test/WeakLabel'


# ---------------------------------------------------------------------------------------------------------------------
# the restatement reproduces the fixture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["A", "B"])
def test_restatement_reproduces_the_reference_run(g21, tag, tmp_path):
    from weasal_amd.ply import write_ply
    g = g21
    n, lv, ign, get = _case(g, tag)
    minima = list(g[tag + "/minima"])
    steps, ended = ref.run_rule(minima, 1)
    assert ended and [(c, r) for _, c, r in steps] == [(False, False), (True, False), (False, False), (True, True)]
    # votes: the reference's float64 smoothing over torch's float32 softmax.  The softmax is a library call whose last bit
    # may depend on the machine, so the replayed votes are held to 1e-7 (a vote is a sum of at most 20 * 0.05 * p with p
    # good to about 1e-7 relative) and everything after them starts from the recorded votes and is held to equality.
    votes = [np.zeros((int(s), len(lv) - len(ign))) for s in g[tag + "/cloud_sizes"]]
    for e, checkpoint, _ in steps:
        for k in range(3):
            key = "%s/e%d/b%d/" % (tag, e, k)
            sm = torch.nn.Softmax(1)(torch.from_numpy(g[key + "logits"])).numpy()
            ref.vote_update(votes, sm, g[key + "points"], g[key + "lengths"], g[key + "inds"], g[key + "clouds"], float(g[tag + "/in_radius"]))
        if e == 1:
            for v, want in zip(votes, get("votes_checkpoint")):
                assert np.abs(v - want).max() <= 1e-7 and np.array_equal(v == 0, want == 0)
    for v, want in zip(votes, get("votes_end")):
        assert np.abs(v - want).max() <= 1e-7 and np.array_equal(v == 0, want == 0)
        assert int((want.sum(axis=1) == 0).sum()) >= len(want) // 10                 # sub-points nobody voted on
        s = np.sort(want[want.sum(axis=1) > 0], axis=1)
        assert (s[:, -1] - s[:, -2]).min() > 1e-3                                    # the fixture's condition
    val_prop = g[tag + "/val_proportions"]
    # the checkpoint on the sub clouds, and the one taken again at the end
    for name, state in (("sub_checkpoint", get("votes_checkpoint")), ("sub_end", get("votes_end"))):
        raw, C, IoUs, line = ref.sub_checkpoint(state, get("sub_labels"), lv, ign, val_prop)
        assert np.array_equal(raw, g["%s/conf_%s" % (tag, name)])
        assert C.dtype == np.float32 and np.array_equal(C, g["%s/iou_in_%s" % (tag, name)])
        assert np.array_equal(IoUs, g["%s/iou_%s" % (tag, name)])
        assert line == str(g[tag + "/lines"][0 if name == "sub_checkpoint" else 1])
    # the end
    outs, raw, C, IoUs, line = ref.full_clouds(get("votes_end"), get("proj"), get("full_labels"), lv, ign)
    assert np.array_equal(raw, g[tag + "/conf_full"]) and np.array_equal(C, g[tag + "/iou_in_full"])
    assert np.array_equal(IoUs, g[tag + "/iou_full"]) and line == str(g[tag + "/lines"][2])
    if tag == "A":       # the matrix the pseudo-label file hands to the plot has the ignored label gone, the weak-label one not
        assert np.array_equal(g[tag + "/plot_conf"], C) and str(g[tag + "/plot_suffix"]) == "G21_validation"
    else:
        assert np.array_equal(g[tag + "/plot_conf"], raw)
    for i, (probs, preds, error, _) in enumerate(outs):
        assert np.array_equal(preds, g["%s/preds_%d" % (tag, i)]) and np.array_equal(error, g["%s/error_%d" % (tag, i)])
        assert probs.dtype == np.float64 and ref.sha(probs) == str(g["%s/proj_probs_sha256_%d" % (tag, i)])
    # the files, byte for byte through the project's writer
    names = ["cloud_%d.ply" % i for i in range(n)]
    ref.write_files(str(tmp_path), write_ply, names, get("full_points"), g[tag + "/coord_offset"], outs, get("full_labels"),
                    [str(s) for s in g[tag + "/names"]])
    for i, name in enumerate(names):
        with open(os.path.join(GOLDEN, "test_run", tag, "predictions", name), "rb") as f:
            assert f.read() == (tmp_path / "predictions" / name).read_bytes()
        data = (tmp_path / "probs" / name).read_bytes()
        assert hashlib.sha256(data).hexdigest() == str(g["%s/probs_file_sha256_%d" % (tag, i)])
        assert data.startswith(str(g["%s/probs_header_%d" % (tag, i)]).encode())
    if tag == "A":
        assert list(g["A/probs_fields_0"][:6]) == ['x', 'y', 'z', 'class_0', 'class_1', 'low_vegetation']


def test_kernel_restatement_equals_the_reference_lines(g21):
    """tests/testrun_ref.kernel_outputs (ws_test_outputs as the header states it) against the reference's own lines on the
    fixture: column table instead of np.insert, value table instead of label_map"""
    from weasal_amd import testrun
    for tag in ("A", "B"):
        n, lv, ign, get = _case(g21, tag)
        kept = [i for i, v in enumerate(lv) if v not in ign]
        true_row = testrun.value_rows(lv)
        for votes, proj, targets in list(zip(get("votes_end"), get("proj"), get("full_labels"))) + \
                list(zip(get("votes_end"), [None] * n, get("sub_labels"))):
            want = ref.cloud_outputs(votes, proj, lv, ign, targets)
            got = ref.kernel_outputs(votes, proj, kept, lv, targets, true_row)
            for a, b in zip(want, got[:4]):
                assert np.array_equal(a, b)
            assert got[4].tolist() == [0, 0]


def test_value_rows():
    from weasal_amd import testrun
    assert testrun.value_rows([0, 1, 2, 3]).tolist() == [0, 1, 2, 3]
    assert testrun.value_rows(list(range(9)) + [10]).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 0, 9]       # absent 9 -> row 0
    assert testrun.value_rows([1, 2]).tolist() == [0, 0, 1]
    with pytest.raises(ValueError):
        testrun.value_rows([1, 1])
    with pytest.raises(ValueError):
        testrun.value_rows([-1, 0])


# ---------------------------------------------------------------------------------------------------------------------
# argument checks, found before the device is touched
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_without_a_device():
    import ctypes as C
    from weasal_amd import _lib
    lib = _lib.lib()
    consts = (C.c_int32 * 4)()
    p = C.cast(consts, C.c_void_p)            # a host address: never dereferenced by a call that fails its checks

    def call(votes=p, c=9, m=5, c_all=10, col_of=p, values=p, status=p, targets=None, error=None, true_row=None, confusion=None):
        rc = lib.ws_test_outputs(votes, 100, c, None, m, col_of, values, c_all, targets, true_row, 11, None, None, error, confusion,
                                 status, None)
        return rc, (lib.ws_last_error() or b"").decode()

    UNSUPPORTED, INVALID = 2, 1
    rc, msg = call(c=9, c_all=65)
    assert rc == UNSUPPORTED and "c_all=65" in msg
    rc, msg = call(c=11, c_all=10)
    assert rc == UNSUPPORTED and "c=11" in msg
    assert call(votes=None)[0] == INVALID and "NULL" in call(votes=None)[1]
    assert call(col_of=None)[0] == INVALID and call(values=None)[0] == INVALID and call(status=None)[0] == INVALID
    assert call(error=p)[0] == INVALID                      # an error map without targets
    assert call(confusion=p, targets=p)[0] == INVALID       # a confusion without true_row
    assert call(c=0)[0] == INVALID and call(m=-1)[0] == INVALID
    assert call(m=0)[0] == 0                                 # nothing queued
    assert call(m=0, votes=None, status=None)[0] == 0
    with pytest.raises(_lib.WeasalHipError, match="c_all=65"):
        _lib.check(call(c_all=65)[0])
