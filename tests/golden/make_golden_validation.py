"""Generates tests/golden/g19_validation.npz (build container only): the reference's own per-epoch validation routine,
utils/trainer_PseudoLabel.py:313-566 (`ModelTrainer.cloud_segmentation_validation`), run on the CPU over stored logits.
The trainer is made with object.__new__, the loader, dataset and network are stubs that hand the routine stored arrays,
torch.cuda.synchronize is a no-op in this process, the matrix handed to the module's IoU_from_confusions is captured by
wrapping that name, and conf_matrix.plot is stubbed.  Everything recorded is data: the inputs, the votes after each epoch
(float64, as the reference keeps them), the summed raw confusion, the balanced matrix, the IoUs, val_proportions, the
val_IoUs.txt text and, for case A, the conf.txt matrix of the `checkpoint_gap` branch.

Case A (DALES): label_values [0..8, 10], 10 ignored, 9 logit columns, truth POSITIONS 0..9 -- position 9 is in the fixture, so
that fast_confusion's label_map on a position (9 -> row 0) is pinned.  Two clouds (400 and 300 points), two epochs of three
batches of four spheres on tiles [0, 1, 0, 0], lengths 2..120 (the reference's fast_confusion squeezes a sphere of ONE row to
a 0-d array and raises, so the routine itself has no such sphere), ascending indices drawn without replacement: the spheres of
tile 0 overlap two- and three-fold.  Case B: label_values 0..3, nothing ignored, one cloud.
Logits: normal * 2, redrawn until every row's two largest float32 softmax values differ by more than 1e-3."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
import utils.trainer_PseudoLabel as T  # noqa: E402  (the reference's own file)

torch.cuda.synchronize = lambda *a, **k: None
T.conf_matrix.plot = lambda *a, **k: None
captured = []
_iou = T.IoU_from_confusions


def _wrapped(C):
    captured.append(np.array(C, copy=True))
    return _iou(C)


T.IoU_from_confusions = _wrapped


def draw_logits(rng, n, c):
    out = np.zeros((n, c), np.float32)
    todo = np.arange(n)
    while len(todo):
        out[todo] = (rng.standard_normal((len(todo), c)) * 2).astype(np.float32)
        l = out[todo]
        e = np.exp(l - l.max(axis=1, keepdims=True), dtype=np.float32)
        p = np.sort(e / e.sum(axis=1, keepdims=True, dtype=np.float32), axis=1)
        todo = todo[(p[:, -1] - p[:, -2]) <= 1e-3]
    return out


class Batch:
    def __init__(self, logits, labels, lengths, inds, clouds):
        self.logits = torch.from_numpy(logits)
        self.labels = torch.from_numpy(labels)
        self.lengths = [torch.from_numpy(lengths)]
        self.input_inds = torch.from_numpy(inds)
        self.cloud_inds = torch.from_numpy(clouds)

    def to(self, device):
        return self


def run_case(tag, rng, label_values, ignored, cloud_sizes, tiles, full_sizes, out, checkpoint):
    label_values = np.asarray(label_values, np.int64)
    n_all = len(label_values)
    c = n_all - len(ignored)
    ds = types.SimpleNamespace(
        validation_split=1, all_splits=[0, 1], num_classes=n_all, label_values=label_values, ignored_labels=np.asarray(ignored, np.int64),
        input_labels=[np.zeros(n, np.int64) for n in cloud_sizes], use_potentials=False,
        validation_labels=[label_values[rng.integers(0, n_all, size=m)].astype(np.int32) for m in full_sizes],
        test_proj=[rng.integers(0, n, size=m).astype(np.int64) for n, m in zip(cloud_sizes, full_sizes)],
        files=["cloud_%d.ply" % i for i in range(len(cloud_sizes))], load_evaluation_points=lambda f: None,
        name="G19", set="validation", label_to_names={int(v): "class_%d" % v for v in label_values})
    tmp = tempfile.mkdtemp()
    cfg = types.SimpleNamespace(num_classes=c, validation_size=3, saving=True, saving_path=tmp, checkpoint_gap=2, dataset="G19")
    tr = object.__new__(T.ModelTrainer)
    tr.device = torch.device("cpu")
    tr.al_iteration = 0
    for i, (n, m) in enumerate(zip(cloud_sizes, full_sizes)):
        out["%s/full_labels_%d" % (tag, i)] = ds.validation_labels[i]
        out["%s/proj_%d" % (tag, i)] = ds.test_proj[i].astype(np.int32)
    for epoch in range(2):
        batches = []
        for k in range(3):
            lengths = rng.integers(2, 121, size=len(tiles)).astype(np.int32)
            if epoch == 0 and k == 0:
                lengths[0], lengths[-1] = 2, 120
            inds = np.concatenate([np.sort(rng.choice(cloud_sizes[t], size=int(n), replace=False)) for t, n in zip(tiles, lengths)])
            n = int(lengths.sum())
            b = Batch(draw_logits(rng, n, c), rng.integers(0, n_all, size=n).astype(np.int64), lengths, inds.astype(np.int64),
                      np.asarray(tiles, np.int32))
            batches.append(b)
            key = "%s/e%d/b%d/" % (tag, epoch, k)
            out[key + "logits"] = b.logits.numpy()
            out[key + "labels"] = b.labels.numpy().astype(np.int32)
            out[key + "lengths"] = lengths
            out[key + "inds"] = inds.astype(np.int32)
            out[key + "clouds"] = np.asarray(tiles, np.int32)
        loader = type("Loader", (), {"dataset": ds, "__iter__": lambda self: iter(batches)})()
        tr.epoch = epoch if checkpoint else 2 * epoch       # (epoch + 1) % checkpoint_gap == 0 in the second epoch of case A only
        del captured[:]
        tr.cloud_segmentation_validation(lambda batch, config: batch.logits, loader, cfg)
        assert all(p.dtype == np.float64 for p in tr.validation_probs)
        balanced = captured[0]
        out["%s/e%d/balanced" % (tag, epoch)] = balanced
        out["%s/e%d/iou" % (tag, epoch)] = _iou(balanced)
        for i, p in enumerate(tr.validation_probs):
            out["%s/e%d/probs_%d" % (tag, epoch, i)] = p.copy()
        # the summed raw confusion of the epoch, by the routine's own lines (:424-442) on the same arrays
        raw = np.zeros((n_all, n_all), np.int64)
        for b in batches:
            probs = torch.nn.Softmax(1)(b.logits).numpy()
            i0 = 0
            for n in b.lengths[0].numpy():
                pr = probs[i0:i0 + n]
                for l_ind, label_value in enumerate(label_values):
                    if label_value in ds.ignored_labels:
                        pr = np.insert(pr, l_ind, 0, axis=1)
                preds = label_values[np.argmax(pr, axis=1)]
                raw += T.fast_confusion(b.labels.numpy()[i0:i0 + n], preds, label_values)
                i0 += n
        Cm = raw.astype(np.float32)
        for l_ind, label_value in reversed(list(enumerate(label_values))):
            if label_value in ds.ignored_labels:
                Cm = np.delete(np.delete(Cm, l_ind, axis=0), l_ind, axis=1)
        Cm *= np.expand_dims(tr.val_proportions / (np.sum(Cm, axis=1) + 1e-6), 1)
        assert np.array_equal(Cm, balanced), "the raw confusion does not lead to the matrix the routine passed on"
        out["%s/e%d/raw" % (tag, epoch)] = raw
    out["%s/val_proportions" % tag] = tr.val_proportions
    out["%s/label_values" % tag] = label_values
    out["%s/ignored" % tag] = np.asarray(ignored, np.int64)
    out["%s/cloud_sizes" % tag] = np.asarray(cloud_sizes, np.int64)
    out["%s/val_IoUs_txt" % tag] = np.array(open(os.path.join(tmp, "val_IoUs.txt")).read())
    if checkpoint:
        out["%s/conf_txt" % tag] = np.loadtxt(os.path.join(tmp, "val_preds_0_2", "conf.txt"), dtype=np.int64)
        for p in tr.validation_probs:           # the arg-max of the votes must not hang on float32 rounding either
            s = np.sort(p[p.sum(axis=1) > 0], axis=1)
            assert (s[:, -1] - s[:, -2]).min() > 1e-5, (s[:, -1] - s[:, -2]).min()
    mult = []
    for epoch in range(2):
        for k in range(3):
            key = "%s/e%d/b%d/" % (tag, epoch, k)
            lengths, inds = out[key + "lengths"], out[key + "inds"]
            mult.append(int(np.bincount(np.concatenate([inds[o:o + n] for o, n, t in
                                                        zip(np.cumsum(lengths) - lengths, lengths, tiles) if t == 0])).max()))
    print(tag, "rows:", sum(int(out["%s/e%d/b%d/lengths" % (tag, e, k)].sum()) for e in range(2) for k in range(3)),
          "largest number of spheres sharing a point, per batch:", mult, "labels seen:", np.unique(out["%s/e0/b0/labels" % tag]))


out = {}
rng = np.random.default_rng(19)
run_case("A", rng, list(range(9)) + [10], [10], [400, 300], [0, 1, 0, 0], [900, 700], out, checkpoint=True)
run_case("B", rng, [0, 1, 2, 3], [], [150], [0, 0, 0, 0], [300], out, checkpoint=False)
path = os.path.join(HERE, "g19_validation.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
