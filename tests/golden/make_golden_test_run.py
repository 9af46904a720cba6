"""Generates tests/golden/g21_test_run.npz and tests/golden/test_run/ (build container only): the reference's own test run,
`ModelTesterPL.cloud_segmentation_test` of utils/tester_PseudoLabel.py:87-449 (case A) and utils/tester_WeakLabel.py:87-485
(case B), run on the CPU over stored logits.  The tester is made with object.__new__, the loader, dataset and network are
stubs that hand the routine stored arrays, torch.cuda.synchronize is a no-op in this process, conf_matrix.plot is stubbed
(it records the matrix it is given), cwd is a temp dir.  The names write_ply, fast_confusion and IoU_from_confusions of
the reference's module are wrapped so that what passes through them is recorded; the files are the ones it wrote.

The stub loader scripts dataset.min_potentials per test epoch: 0.3, 0.7, 1.2, 1.8.  With num_votes = 1 the rule
(:220-223, :268, :446) gives: no checkpoint; a checkpoint on the sub clouds (last_min 0.5); none; a checkpoint (last_min
1.5 > 1) that is the end.

Case A (DALES): label_values [0..8, 10], 10 ignored, 9 logit columns; two clouds of 400 and 300 sub-points, 900 and 700 full
points, three batches of four spheres per epoch on tiles [0, 1, 0, 0], lengths 2..40, ascending indices drawn without
replacement from the first nine tenths of a cloud (the last tenth is never voted on; the spheres of tile 0 overlap), points
uniform in [-0.8, 0.8]^3 around the centre with in_radius 1 (the 0.7 mask cuts some), coord_offset non-zero.
Case B: label_values 0..3, nothing ignored, one cloud, the network returns a triple.
Logits: 2 * normal + 5 on the class drawn for the sub-point.  The whole case is redrawn until every voted row of the float64
votes, at the checkpoint and at the end, has its two largest values more than 1e-3 apart; that is asserted.

The probs/ files and the expanded rows they hold are float64 and large: they are recorded as their field layout and SHA-256
digests (the restatement in tests/testrun_ref.py rebuilds the same bytes from the recorded votes)."""
import contextlib
import hashlib
import io
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
import utils.tester_PseudoLabel as TP  # noqa: E402  (the reference's own files)
import utils.tester_WeakLabel as TW  # noqa: E402

torch.cuda.synchronize = lambda *a, **k: None
MINIMA = [0.3, 0.7, 1.2, 1.8]
IN_RADIUS = 1.0


class Batch:
    def __init__(self, logits, points, lengths, inds, clouds):
        self.logits = torch.from_numpy(logits)
        self.points = [torch.from_numpy(points)]
        self.lengths = [torch.from_numpy(lengths)]
        self.input_inds = torch.from_numpy(inds)
        self.cloud_inds = torch.from_numpy(clouds)

    def to(self, device):
        return self


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(tag, T, rng, label_values, ignored, cloud_sizes, tiles, full_sizes, triple, out, file_dir):
    label_values = np.asarray(label_values, np.int64)
    n_all = len(label_values)
    kept = [v for v in label_values if v not in ignored]
    c = len(kept)
    names = ["cloud_%d" % i for i in range(len(cloud_sizes))]
    klass = [rng.integers(0, c, size=n) for n in cloud_sizes]                       # the column the logits favour
    ds = types.SimpleNamespace(
        num_classes=n_all, label_values=label_values, ignored_labels=np.asarray(ignored, np.int64),
        input_labels=[np.where(rng.random(n) < 0.7, np.asarray(kept)[k], label_values[rng.integers(0, n_all, size=n)]).astype(np.int32)
                      for n, k in zip(cloud_sizes, klass)],
        test_proj=[rng.integers(0, n, size=m).astype(np.int64) for n, m in zip(cloud_sizes, full_sizes)],
        files=["data/" + n + ".ply" for n in names], cloud_names=names, name="G21", set="validation",
        label_to_names={int(v): ("class %d" % v if v != 2 else "low  vegetation") for v in label_values},
        coord_offset=np.array([[100.5, -20.25, 3.0]], np.float32),
        # cloud i's smallest potential is the last scripted minimum + 0.25 i: a replay can serve the earlier minima by
        # lowering these arrays and ends on them as they are written
        potentials=[torch.from_numpy(np.concatenate([[0.0], 0.01 + rng.random(19 + i)]) + MINIMA[-1] + 0.25 * i) for i in range(len(cloud_sizes))],
        pot_trees=[types.SimpleNamespace(data=rng.random((20 + i, 3))) for i in range(len(cloud_sizes))],
        min_potentials=None)
    # the full-resolution targets hold no ignored label: utils/conf_matrix.py:52-56 stops in a debugger on one (the sub-cloud
    # labels above do hold some: fast_confusion counts them in the row that is deleted)
    ds.validation_labels = [np.asarray(kept)[np.where(rng.random(m) < 0.8, k[p], rng.integers(0, c, size=m))].astype(np.int32)
                            for k, p, m in zip(klass, ds.test_proj, full_sizes)]
    full_points = {f: (rng.random((m, 3)) * 50).astype(np.float32) for f, m in zip(ds.files, full_sizes)}
    ds.load_evaluation_points = lambda f: full_points[f]

    epochs = []
    for e in range(len(MINIMA)):
        batches = []
        for k in range(3):
            lengths = rng.integers(2, 41, size=len(tiles)).astype(np.int32)
            inds = np.concatenate([np.sort(rng.choice(cloud_sizes[t] * 9 // 10, size=int(n), replace=False)) for t, n in zip(tiles, lengths)])
            n = int(lengths.sum())
            fav = np.concatenate([klass[t][inds[o:o + m]] for t, o, m in zip(tiles, np.cumsum(lengths) - lengths, lengths)])
            logits = (rng.standard_normal((n, c)) * 2).astype(np.float32)
            logits[np.arange(n), fav] += 5
            points = rng.uniform(-0.8, 0.8, size=(n, 3)).astype(np.float32)
            batches.append(Batch(logits, points, lengths, inds.astype(np.int64), np.asarray(tiles, np.int32)))
        epochs.append(batches)

    class Loader:
        dataset = ds
        epoch = 0

        def __iter__(self):
            e = self.epoch
            Loader.epoch += 1
            for b in epochs[e]:
                yield b
            ds.min_potentials = torch.tensor([MINIMA[e] + 0.25 * i for i in range(len(cloud_sizes))])

    cfg = types.SimpleNamespace(num_classes=c, validation_size=3, saving=True, saving_path="results/Log_g21_" + tag, in_radius=IN_RADIUS)
    tester = object.__new__(T.ModelTesterWL if triple else T.ModelTesterPL)
    tester.device = torch.device("cpu")
    rec = dict(iou_in=[], votes=[], plys=[], fast=[], plot=[])
    real_iou, real_fast, real_ply = T.IoU_from_confusions, T.fast_confusion, T.write_ply

    def w_iou(C):
        rec["iou_in"].append(np.array(C, copy=True))
        rec["votes"].append([p.copy() for p in tester.test_probs])
        return real_iou(C)

    def w_fast(*a):
        r = real_fast(*a)
        rec["fast"].append(np.array(r, copy=True))
        return r

    def w_ply(name, fields, field_names):
        rec["plys"].append((name, [np.array(f, copy=True) for f in fields], list(field_names)))
        return real_ply(name, fields, field_names)

    T.IoU_from_confusions, T.fast_confusion, T.write_ply = w_iou, w_fast, w_ply
    T.conf_matrix.plot = lambda Confs, *a, **k: rec["plot"].append((np.array(Confs, copy=True), k.get("file_suffix")))
    net = (lambda batch, config: (batch.logits, None, None)) if triple else (lambda batch, config: batch.logits)
    tmp = tempfile.mkdtemp()
    cwd = os.getcwd()
    os.chdir(tmp)
    text = io.StringIO()
    try:
        with contextlib.redirect_stdout(text):
            tester.cloud_segmentation_test(net, Loader(), cfg, num_votes=1)
    finally:
        os.chdir(cwd)
        T.IoU_from_confusions, T.fast_confusion, T.write_ply = real_iou, real_fast, real_ply
    assert Loader.epoch == 4 and len(rec["iou_in"]) == 3, (Loader.epoch, len(rec["iou_in"]))    # sub, sub (at the end), full
    assert all(p.dtype == np.float64 for p in tester.test_probs)
    for state in (rec["votes"][0], rec["votes"][2]):
        for p in state:
            s = np.sort(p[p.sum(axis=1) > 0], axis=1)
            if (s[:, -1] - s[:, -2]).min() <= 1e-3:
                shutil.rmtree(tmp)
                return False
    n_clouds = len(cloud_sizes)
    lines = [l for l in text.getvalue().split("\n") if " | " in l]
    assert len(lines) == 3
    out[tag + "/lines"] = np.array(lines)
    out[tag + "/stdout"] = np.array(text.getvalue())
    for i in range(n_clouds):
        out["%s/sub_labels_%d" % (tag, i)] = ds.input_labels[i]
        out["%s/full_labels_%d" % (tag, i)] = ds.validation_labels[i]
        out["%s/proj_%d" % (tag, i)] = ds.test_proj[i].astype(np.int32)
        out["%s/full_points_%d" % (tag, i)] = full_points[ds.files[i]]
        out["%s/pot_points_%d" % (tag, i)] = np.asarray(ds.pot_trees[i].data)
        out["%s/potentials_%d" % (tag, i)] = ds.potentials[i].numpy()
        out["%s/votes_checkpoint_%d" % (tag, i)] = rec["votes"][0][i]
        out["%s/votes_end_%d" % (tag, i)] = rec["votes"][2][i]
        assert int((rec["votes"][2][i].sum(axis=1) == 0).sum()) >= cloud_sizes[i] // 10
    for e, batches in enumerate(epochs):
        for k, b in enumerate(batches):
            key = "%s/e%d/b%d/" % (tag, e, k)
            out[key + "logits"] = b.logits.numpy()
            out[key + "points"] = b.points[0].numpy()
            out[key + "lengths"] = b.lengths[0].numpy()
            out[key + "inds"] = b.input_inds.numpy().astype(np.int32)
            out[key + "clouds"] = b.cloud_inds.numpy()
    # fast_confusion calls: n_clouds per sub-cloud checkpoint (two of them), n_clouds on the full clouds (+ n_clouds more
    # in the weak-label file, whose saving loop calls it again)
    fast = rec["fast"]
    out[tag + "/conf_sub_checkpoint"] = np.sum(fast[:n_clouds], axis=0)
    out[tag + "/conf_sub_end"] = np.sum(fast[n_clouds:2 * n_clouds], axis=0)
    out[tag + "/conf_full"] = np.sum(fast[2 * n_clouds:3 * n_clouds], axis=0)
    for name, C in zip(("sub_checkpoint", "sub_end", "full"), rec["iou_in"]):
        out["%s/iou_in_%s" % (tag, name)] = C
        out["%s/iou_%s" % (tag, name)] = real_iou(C)
    out[tag + "/plot_conf"] = rec["plot"][0][0]
    out[tag + "/plot_suffix"] = np.array(rec["plot"][0][1])
    val_prop = np.zeros(c, np.float32)
    for i, v in enumerate(kept):
        val_prop[i] = np.sum([np.sum(l == v) for l in ds.validation_labels])
    out[tag + "/val_proportions"] = val_prop
    out[tag + "/label_values"] = label_values
    out[tag + "/ignored"] = np.asarray(ignored, np.int64)
    out[tag + "/names"] = np.array([ds.label_to_names[int(v)] for v in label_values])
    out[tag + "/coord_offset"] = ds.coord_offset
    out[tag + "/cloud_sizes"] = np.asarray(cloud_sizes, np.int64)
    out[tag + "/in_radius"] = np.float64(IN_RADIUS)
    out[tag + "/minima"] = np.asarray(MINIMA)
    out[tag + "/saving_path"] = np.array(cfg.saving_path)
    root = os.path.join(tmp, "test", "WeakLabel" if triple else "PseudoLabel", cfg.saving_path.split("/")[-1])
    for name, fields, field_names in rec["plys"]:
        kind, cloud = name.split("/")[-2:]
        i = names.index(cloud[:-4])
        if kind == "predictions":
            out["%s/preds_%d" % (tag, i)], out["%s/error_%d" % (tag, i)] = fields[1], fields[3]
            assert fields[1].dtype == np.int32 and fields[3].dtype == np.int8 and field_names == ['x', 'y', 'z', 'preds', 'targets', 'error']
        elif kind == "probs":
            assert fields[1].dtype == np.float64 and fields[1].shape == (full_sizes[i], n_all)
            out["%s/proj_probs_sha256_%d" % (tag, i)] = np.array(sha(fields[1]))
            out["%s/probs_file_sha256_%d" % (tag, i)] = np.array(hashlib.sha256(open(os.path.join(root, "probs", cloud), "rb").read()).hexdigest())
            out["%s/probs_fields_%d" % (tag, i)] = np.array(field_names)
            with open(os.path.join(root, "probs", cloud), "rb") as f:
                out["%s/probs_header_%d" % (tag, i)] = np.array(f.read().split(b"end_header\n")[0].decode() + "end_header\n")
    for kind in ("predictions", "potentials"):
        dst = os.path.join(file_dir, tag, kind)
        os.makedirs(dst, exist_ok=True)
        for n in names:
            shutil.copy(os.path.join(root, kind, n + ".ply"), os.path.join(dst, n + ".ply"))
    shutil.rmtree(tmp)
    return True


def main():
    file_dir = os.path.join(HERE, "test_run")
    if os.path.exists(file_dir):
        shutil.rmtree(file_dir)
    out = {}
    cases = (("A", TP, list(range(9)) + [10], [10], [400, 300], [0, 1, 0, 0], [900, 700], False),
             ("B", TW, [0, 1, 2, 3], [], [150], [0, 0, 0, 0], [300], True))
    for tag, T, lv, ign, sizes, tiles, full, triple in cases:
        for attempt in range(2000):
            rng = np.random.default_rng([21, ord(tag), attempt])
            if run_case(tag, T, rng, lv, ign, sizes, tiles, full, triple, out, file_dir):
                print(tag, "drawn at attempt", attempt)
                break
        else:
            raise SystemExit("no draw of case %s keeps the two largest votes of every row 1e-3 apart" % tag)
    path = os.path.join(HERE, "g21_test_run.npz")
    np.savez_compressed(path, **out)
    files = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(file_dir) for f in fs)
    print("wrote", path, os.path.getsize(path), "bytes;", file_dir, files, "bytes")


main()
