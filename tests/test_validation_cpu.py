"""Per-epoch validation, the parts that need no GPU: the numpy restatement (tests/validation_ref.py) reproduces
tests/golden/g19_validation.npz, written by the reference's own `cloud_segmentation_validation`
(tests/golden/make_golden_validation.py); `validation.confusion_tables` is `fast_confusion`'s map; the new C entry
validates its arguments before it touches the device."""
import ctypes as C

import numpy as np
import pytest

import validation_ref as ref
from conftest import golden

CASES = ("A", "B")


def batches(g, tag, epoch):
    for k in range(3):
        key = "%s/e%d/b%d/" % (tag, epoch, k)
        yield {f: g[key + f] for f in ("logits", "labels", "lengths", "inds", "clouds")}


@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_the_reference_routine(tag):
    g = golden("g19_validation.npz")
    lv, ign = g[tag + "/label_values"], g[tag + "/ignored"]
    sizes = g[tag + "/cloud_sizes"]
    full = [g["%s/full_labels_%d" % (tag, i)] for i in range(len(sizes))]
    prop = ref.proportions(full, lv, ign)
    assert prop.dtype == np.float32 and np.array_equal(prop, g[tag + "/val_proportions"])
    votes = [np.zeros((int(n), len(lv) - len(ign))) for n in sizes]
    for epoch in range(2):
        conf = np.zeros((len(lv), len(lv)), np.int64)
        for b in batches(g, tag, epoch):
            ref.vote_batch(votes, b["logits"], b["lengths"], b["inds"], b["clouds"])
            conf += ref.batch_confusion(b["logits"], b["labels"], lv, ign)
        for i, p in enumerate(votes):
            assert np.abs(p - g["%s/e%d/probs_%d" % (tag, epoch, i)]).max() <= 1e-12
        assert np.array_equal(conf, g["%s/e%d/raw" % (tag, epoch)])
        Cm = ref.balanced(conf, lv, ign, prop)
        assert np.array_equal(Cm, g["%s/e%d/balanced" % (tag, epoch)])
        assert np.array_equal(ref.iou(Cm), g["%s/e%d/iou" % (tag, epoch)])
    if tag == "A":
        assert conf[0, :].sum() > conf[1:9, :].sum(axis=1).max()        # position 9 ("Ignore") is counted in row 0: the quirk
        assert conf[9, :].sum() == 0
        projs = [g["A/proj_%d" % i] for i in range(len(sizes))]
        assert np.array_equal(ref.reprojected_confusion(votes, projs, full, lv, ign), g["A/conf_txt"])


LABEL_SETS = [(list(range(9)) + [10], [10]), ([0, 1, 2, 3, 5, 6, 7, 8, 10], [0]), ([0, 1, 2, 3], []), ([2, 5, 9], [])]


@pytest.mark.parametrize("label_values, ignored", LABEL_SETS)
def test_confusion_tables_are_fast_confusions_map(label_values, ignored):
    """truth positions and predicted label values through the tables == fast_confusion(truth, preds, label_values)"""
    from weasal_amd import tester, validation
    lv = np.asarray(label_values, np.int64)
    true_row, pred_row, kept = validation.confusion_tables(lv, ignored)
    n, c = len(lv), len(lv) - len(ignored)
    assert true_row.dtype == np.int32 and pred_row.dtype == np.int32 and true_row.shape == (n,) and pred_row.shape == (c,)
    assert kept == [k for k, v in enumerate(label_values) if v not in ignored]
    rng = np.random.default_rng(5)
    truth = rng.integers(0, n, size=4000).astype(np.int64)
    cols = rng.integers(0, c, size=4000)
    preds = lv[np.asarray(kept)[cols]]                        # label_values[argmax of the probabilities with zero columns inserted]
    want = tester.fast_confusion(truth, preds, lv)
    got = np.zeros((n, n), np.int64)
    np.add.at(got, (true_row[truth], pred_row[cols]), 1)
    assert np.array_equal(got, want)
    assert ref.label_rows(lv, ignored) == (list(true_row), list(pred_row), kept)
    if label_values[-1] == 10 and ignored == [10]:
        assert true_row[9] == 0                               # DALES: position 9 goes through label_map[9] = 0


def test_overlap_masks_from_centres():
    from weasal_amd import validation
    tiles = [0, 1, 0, 0]
    centres = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0], [9, 0, 0]], np.float64)
    m = validation.overlap_from_centres(tiles, centres, 2.0)
    assert m.dtype == np.uint64 and list(m) == [0b0100, 0, 0b0001, 0]
    assert list(validation.overlap_from_centres(tiles, centres, 5.0)) == [0b1100, 0, 0b1001, 0b0101]
    with pytest.raises(ValueError):
        validation.overlap_from_centres([0] * 65, np.zeros((65, 3)), 1.0)


def test_val_iou_line_format(tmp_path):
    from weasal_amd import validation
    g = golden("g19_validation.npz")
    path = tmp_path / "val_IoUs.txt"
    for epoch in range(2):
        validation.append_val_IoUs(str(path), g["A/e%d/iou" % epoch])
    assert open(path).read() == str(g["A/val_IoUs_txt"])


def test_potentials_go_through_the_ply_writer(tmp_path):
    """(:481-494) x, y, z and `pots` as float32, one file per cloud named after the tile"""
    import types

    import torch
    from weasal_amd import ply, validation
    rng = np.random.default_rng(2)
    pts = [rng.random((n, 3)).astype(np.float32) for n in (7, 4)]
    pots = [rng.random(n) for n in (7, 4)]                                   # float64, as the sampler keeps them
    sampler = types.SimpleNamespace(pot_points=[torch.from_numpy(p) for p in pts], potentials=[torch.from_numpy(p) for p in pots])
    validation.save_potentials(str(tmp_path / "potentials"), ["data/tile_a.ply", "tile_b.ply"], sampler)
    for name, p, v in zip(("tile_a.ply", "tile_b.ply"), pts, pots):
        back = ply.read_ply(str(tmp_path / "potentials" / name))
        assert back.dtype.names == ("x", "y", "z", "pots") and back["pots"].dtype == np.float32
        assert np.array_equal(np.stack([back["x"], back["y"], back["z"]], axis=1), p)
        assert np.array_equal(back["pots"], v.astype(np.float32))
    with pytest.raises(ValueError):
        validation.save_potentials(str(tmp_path / "potentials"), ["only_one.ply"], sampler)


def test_status_words_are_named():
    from weasal_amd import _lib, validation
    k = _lib.ABI.constants
    validation.raise_on_status([0, 0, 0])
    with pytest.raises(ValueError, match="3 rows that do not ascend"):
        validation.raise_on_status([3, 0, 0])
    with pytest.raises(ValueError, match="2 point ids outside.*7 values outside"):
        validation.raise_on_status([0, 2, 7])
    assert validation.STATUS_WORDS == 3 and k["WS_PYRAMID_MAX_BATCH"] == 64


def _entry(**over):
    """ws_validation_update(logits, n, c, ld, input_inds, labels, points, radius_mask, h_offsets, h_lens, h_clouds, h_overlap,
    nb, votes, cloud_rows, n_clouds, smooth, true_row, n_true, pred_row, nc, confusion, status, stream)"""
    from weasal_amd import _lib
    one = C.c_void_p(16)      # never dereferenced: validation fails first
    host = lambda a: (a, C.c_void_p(a.ctypes.data))
    keep = [host(np.array([0, 3], np.int64)), host(np.array([3, 5], np.int32)), host(np.array([0, 1], np.int32)),
            host(np.array([0, 0], np.uint64))]
    args = dict(logits=one, n=8, c=9, ld=9, input_inds=one, labels=one, points=None, radius_mask=0.0, h_offsets=keep[0][1],
                h_lens=keep[1][1], h_clouds=keep[2][1], h_overlap=keep[3][1], nb=2, votes=one, cloud_rows=one, n_clouds=2,
                smooth=0.95, true_row=one, n_true=10, pred_row=one, nc=10, confusion=one, status=one, stream=None)
    for name, v in over.items():
        if isinstance(v, np.ndarray):
            keep.append(host(v))
            v = keep[-1][1]
        args[name] = v
    lib = _lib.lib()
    return lib.ws_validation_update(*args.values()), lib.ws_last_error()


def test_entry_validates_before_touching_the_device():
    INVALID, UNSUPPORTED = 1, 2
    for over, want in (({"nb": 0}, INVALID), ({"nb": 65}, UNSUPPORTED), ({"c": 0}, INVALID), ({"c": 65, "ld": 65}, UNSUPPORTED),
                       ({"nc": 0}, INVALID), ({"nc": 65}, UNSUPPORTED), ({"n": -1}, INVALID), ({"ld": 8}, INVALID),
                       ({"n_clouds": 0}, INVALID), ({"n_true": 0}, INVALID), ({"n": 1 << 31}, UNSUPPORTED)):
        rc, _ = _entry(**over)
        assert rc == want, over
    assert _entry(n=0, logits=None, input_inds=None, votes=None, status=None)[0] == 0            # nothing to do: no launch
    for name in ("logits", "input_inds", "h_offsets", "h_lens", "h_clouds", "h_overlap", "votes", "cloud_rows", "status", "true_row",
                 "pred_row", "confusion"):
        rc, msg = _entry(**{name: None})
        assert rc == INVALID and b"NULL" in msg, name
    rc, msg = _entry(radius_mask=0.5)
    assert rc == INVALID and b"points" in msg
    # the host arrays are checked where they stand
    assert _entry(h_lens=np.array([3, 6], np.int32))[0] == INVALID                                # past the last row
    assert _entry(h_offsets=np.array([0, 2], np.int64))[0] == INVALID                             # overlaps the sphere before
    assert _entry(h_lens=np.array([-1, 5], np.int32))[0] == INVALID
    rc, msg = _entry(h_clouds=np.array([0, 2], np.int32))
    assert rc == INVALID and b"cloud 2" in msg
    assert _entry(h_clouds=np.array([-1, 0], np.int32))[0] == INVALID
    assert _entry(h_overlap=np.array([4, 0], np.uint64))[0] == INVALID                            # names a third sphere of two
    rc, msg = _entry(h_overlap=np.array([2, 0], np.uint64))
    assert rc == INVALID and b"disagree" in msg                                                  # one-sided pair
