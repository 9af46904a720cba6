"""GPU: ws_test_outputs against tests/testrun_ref.kernel_outputs (EQUAL: every output is a copy, a compare or an integer
count), the test run replayed over tests/golden/g21_test_run.npz (the reference's own routine, both files), a real run on two
small synthetic tiles with a checkpoint of loop.ModelTrainer, and the two active-learning passes."""
import os
import types

import numpy as np
import pytest
import torch

import testrun_ref as ref
from conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu

# csrc/testrun.hip: at most TEST_GRID_CAP = 2048 workgroups, each taking 256 rows at a time (128 when c_all > 53): beyond
# 524 288 points a workgroup strides over the tiles
TEST_GRID = 2048 * 256

LABEL_CASES = {
    "last_ignored": (list(range(9)) + [10], [10]),           # (c, c_all) = (9, 10), DALES
    "first_ignored": (list(range(10)), [0]),                 # (9, 10)
    "two_middle": (list(range(10)), [3, 6]),                 # (8, 10)
    "none_ignored": ([0, 1, 2, 3], []),                      # (4, 4)
    "one_of_two": ([0, 1], [0]),                             # (1, 2)
    "wide": (list(range(64)), [5]),                          # (63, 64): tiles of 128 rows
}


def _dev(gpu, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _votes(rng, n_sub, c):
    """float32 votes the way a pass leaves them, with rows nobody voted on and exact ties of the largest value"""
    v = rng.random((n_sub, c)).astype(np.float32) * 0.3
    v[rng.random(n_sub) < 0.15] = 0                                           # all-zero rows
    tie = np.flatnonzero(rng.random(n_sub) < 0.2)
    if c > 1:
        a, b = rng.integers(0, c, size=len(tie)), rng.integers(0, c, size=len(tie))
        v[tie, a] = 0.5
        v[tie, b] = 0.5                                                       # the first of the two wins
    return v


def _check(gpu, lv, ign, n_sub, m, seed, proj_mode="random", bad_targets=False):
    from weasal_amd import testrun
    rng = np.random.default_rng(seed)
    tables = testrun.LabelTables(lv, ign, gpu)
    lv = np.asarray(lv)
    votes = _votes(rng, n_sub, tables.c)
    if proj_mode == "identity":
        proj, m = None, n_sub
    else:
        proj = rng.integers(0, n_sub, size=m).astype(np.int32)
        if proj_mode == "bad" and m >= 4:
            proj[[0, m // 2]] = -1
            proj[[1, m - 1]] = n_sub
    targets = lv[rng.integers(0, len(lv), size=m)].astype(np.int32)
    if bad_targets and m >= 3:
        targets[0], targets[m // 3], targets[m - 1] = -1, int(lv.max()) + 1, 1 << 20
    true_row = testrun.value_rows(lv)
    kept = tables.kept
    want = ref.kernel_outputs(votes, proj, kept, lv, targets, true_row)
    status = testrun.new_status(gpu)
    conf = torch.zeros((len(lv), len(lv)), dtype=torch.int64, device=gpu)
    d_votes, d_proj, d_targets = _dev(gpu, votes), _dev(gpu, proj), _dev(gpu, targets)
    got = testrun.outputs(d_votes, tables, status, proj=d_proj, targets=d_targets, confusion=conf, probs=True, preds=True, error=True)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[2].dtype == torch.int8
    assert got[0].cpu().numpy().tobytes() == want[0].tobytes()                # bit for bit
    assert np.array_equal(got[1].cpu().numpy(), want[1]) and np.array_equal(got[2].cpu().numpy(), want[2])
    assert np.array_equal(conf.cpu().numpy(), want[3]) and status.cpu().tolist() == want[4].tolist()
    if proj_mode != "bad" and not bad_targets:
        assert want[4].tolist() == [0, 0] and int(want[3].sum()) == m
    return dict(tables=tables, votes=d_votes, proj=d_proj, targets=d_targets, want=want, got=got, conf=conf, status=status,
                host=(votes, proj, kept, lv, targets, true_row))


@pytest.mark.parametrize("labels", sorted(LABEL_CASES))
@pytest.mark.parametrize("m", [1, 257, 3 * 256 - 64, 2 * 256 + 1, 3 * 128 + 1])
def test_kernel_equals_the_restatement(gpu, labels, m):
    """m: one row; one beyond a workgroup; one wave short of a workgroup multiple; one row beyond one (and beyond a multiple
    of the 128-row tile of the wide case)"""
    lv, ign = LABEL_CASES[labels]
    _check(gpu, lv, ign, 300, m, seed=[21, m, len(lv)])


@pytest.mark.parametrize("labels", ["last_ignored", "first_ignored", "wide"])
def test_kernel_identity_projection(gpu, labels):
    lv, ign = LABEL_CASES[labels]
    _check(gpu, lv, ign, 1000, None, seed=5, proj_mode="identity")


def test_kernel_above_the_grid_cap(gpu):
    lv, ign = LABEL_CASES["last_ignored"]
    r = _check(gpu, lv, ign, 5000, TEST_GRID + 257, seed=6)
    assert r["got"][0].shape[0] > TEST_GRID


@pytest.mark.parametrize("labels", ["last_ignored", "first_ignored", "wide"])
def test_kernel_counts_bad_indices_and_targets(gpu, labels):
    """proj entries of -1 and n_sub, targets outside the table: counted, no fault, every other row as without them"""
    lv, ign = LABEL_CASES[labels]
    r = _check(gpu, lv, ign, 300, 700, seed=7, proj_mode="bad", bad_targets=True)
    assert r["want"][4].tolist() == [4, 3]
    clean = _check(gpu, lv, ign, 300, 700, seed=7)
    votes, proj, kept, lv_, targets, true_row = r["host"]
    rows = np.ones(700, bool)
    rows[[0, 350, 1, 699]] = False
    assert np.array_equal(r["want"][1][rows], clean["want"][1][rows]) and (r["want"][1][~rows] == lv_[0]).all()
    assert (r["want"][0][~rows] == 0).all()


def test_kernel_all_zero_votes_predict_the_first_label(gpu):
    from weasal_amd import testrun
    for labels in ("last_ignored", "first_ignored"):
        lv, ign = LABEL_CASES[labels]
        tables = testrun.LabelTables(lv, ign, gpu)
        status = testrun.new_status(gpu)
        probs, preds, _ = testrun.outputs(torch.zeros((50, 9), device=gpu), tables, status, probs=True)
        assert (preds.cpu().numpy() == lv[0]).all() and not probs.any() and status.cpu().tolist() == [0, 0]


def test_kernel_optional_outputs_accumulation_and_determinism(gpu):
    from weasal_amd import testrun
    lv, ign = LABEL_CASES["two_middle"]
    r = _check(gpu, lv, ign, 300, 1500, seed=8, proj_mode="bad", bad_targets=True)
    t, want = r["tables"], r["want"]
    # a second call accumulates into the same confusion and the same status words
    again = testrun.outputs(r["votes"], t, r["status"], proj=r["proj"], targets=r["targets"], confusion=r["conf"], probs=True, error=True)
    assert np.array_equal(r["conf"].cpu().numpy(), 2 * want[3]) and r["status"].cpu().tolist() == (2 * want[4]).tolist()
    for a, b in zip(again, r["got"]):                                         # two runs, the same bits
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    # every optional output left out in turn: the others do not change
    for drop in ("probs", "preds", "error", "confusion", "targets"):
        status = testrun.new_status(gpu)
        conf = None if drop in ("confusion", "targets") else torch.zeros_like(r["conf"])
        targets = None if drop == "targets" else r["targets"]
        got = testrun.outputs(r["votes"], t, status, proj=r["proj"], targets=targets, confusion=conf, probs=drop != "probs",
                              preds=drop != "preds", error=drop not in ("error", "targets"))
        for name, g, w in zip(("probs", "preds", "error"), got, want[:3]):
            if name == drop or (drop == "targets" and name == "error"):
                assert g is None
            else:
                assert g.cpu().numpy().tobytes() == w.tobytes(), (drop, name)
        if conf is not None:
            assert np.array_equal(conf.cpu().numpy(), want[3]) and status.cpu().tolist() == want[4].tolist()
        else:
            assert status.cpu().tolist() == [int(want[4][0]), 0]             # targets are judged only for a confusion
    with pytest.raises(ValueError):
        testrun.outputs(r["votes"], t, r["status"], proj=r["proj"], error=True)
    with pytest.raises(ValueError):
        testrun.raise_on_status(r["status"].cpu())


# ---------------------------------------------------------------------------------------------------------------------
# the golden replay
# ---------------------------------------------------------------------------------------------------------------------
VOTE_BOUND = 20 * 2e-6      # 2e-6 per update (tests/test_tester.py), at most 1 / (1 - 0.95) = 20 of a smoothed vote's weight


class StubNet:
    def __init__(self, triple):
        self.triple = triple

    def to(self, device):
        return self

    def eval(self):
        return self

    def __call__(self, batch, config):
        return (batch["logits"], None, None) if self.triple else batch["logits"]


class StubSampler:
    """serves the scripted minima: the recorded potentials lowered by (last minimum - this epoch's), and as recorded in
    the last epoch"""

    def __init__(self, g, tag, gpu):
        n = len(g[tag + "/cloud_sizes"])
        self.final = [_dev(gpu, g["%s/potentials_%d" % (tag, i)]) for i in range(n)]
        self.pot_points = [_dev(gpu, g["%s/pot_points_%d" % (tag, i)].astype(np.float32)) for i in range(n)]
        self.sub_points = [torch.empty((int(s), 3), device=gpu) for s in g[tag + "/cloud_sizes"]]
        self.minima = [float(v) for v in g[tag + "/minima"]]
        self.potentials = None

    def serve(self, epoch):
        last = epoch == len(self.minima) - 1
        self.potentials = self.final if last else [p - (self.minima[-1] - self.minima[epoch]) for p in self.final]


def _replay(g, tag, gpu, root, cls, set_name="validation", max_test_epochs=6, **kw):
    from weasal_amd import testrun
    n = len(g[tag + "/cloud_sizes"])
    lv, ign = g[tag + "/label_values"], g[tag + "/ignored"]
    get = lambda name: [g["%s/%s_%d" % (tag, name, i)] for i in range(n)]
    full_points = dict(zip(["data/cloud_%d.ply" % i for i in range(n)], get("full_points")))
    ts = testrun.TestSet(["cloud_%d" % i for i in range(n)], list(full_points), lv, ign,
                         {int(v): str(s) for v, s in zip(lv, g[tag + "/names"])}, set_name,
                         [_dev(gpu, p) for p in get("proj")], [_dev(gpu, l) for l in get("full_labels")],
                         [_dev(gpu, l) for l in get("sub_labels")], name="G21", coord_offset=g[tag + "/coord_offset"],
                         load_points=lambda f: full_points[f])
    sampler = StubSampler(g, tag, gpu)
    seen = {}

    def batches(epoch):
        if epoch == 2:                        # the votes the checkpoint after epoch 1 saw
            seen["checkpoint"] = [p.cpu().numpy() for p in tester.votes.probs]
        for k in range(3):
            key = "%s/e%d/b%d/" % (tag, epoch, k)
            yield {"logits": _dev(gpu, g[key + "logits"]), "points": _dev(gpu, g[key + "points"]), "lengths": g[key + "lengths"],
                   "input_inds": _dev(gpu, g[key + "inds"].astype(np.int64)), "cloud_inds": g[key + "clouds"]}
        sampler.serve(epoch)
    cfg = types.SimpleNamespace(in_radius=float(g[tag + "/in_radius"]), saving=True, saving_path=str(g[tag + "/saving_path"]),
                                validation_size=3, class_w=[0.1 * k for k in range(len(lv) - len(ign))], added_labels_per_epoch=7)
    net = StubNet(cls.__name__.endswith("WL"))
    tester = cls(net, cfg, device=gpu)
    result = tester.cloud_segmentation_test(net, sampler, batches, ts, num_votes=1, max_test_epochs=max_test_epochs, root=str(root), **kw)
    return tester, result, seen, get


@pytest.mark.parametrize("tag", ["A", "B"])
def test_golden_replay(gpu, tag, tmp_path, capsys):
    from weasal_amd import testrun
    from weasal_amd.ply import read_ply
    g = golden("g21_test_run.npz")
    cls = testrun.ModelTester if tag == "A" else testrun.ModelTesterWL
    tester, res, seen, get = _replay(g, tag, gpu, tmp_path, cls)
    out = capsys.readouterr().out
    n = len(get("proj"))
    lv, ign = g[tag + "/label_values"], g[tag + "/ignored"]
    # ---- the loop
    assert tester.test_epochs == 4 and tester.checkpoints == 2 and tester._sync_count == 4 + 2 + 1
    assert tester.minima[-1] == 1.8 and [round(v, 6) for v in tester.minima] == [0.3, 0.7, 1.2, 1.8]
    # ---- votes against the float64 golden
    for name, got in (("votes_checkpoint", seen["checkpoint"]), ("votes_end", [p.cpu().numpy() for p in tester.votes.probs])):
        for v, want in zip(got, get(name)):
            err = np.abs(v.astype(np.float64) - want).max()
            print(tag, name, "max |vote - float64 golden| = %.3g (bound %.3g)" % (err, VOTE_BOUND))
            assert err <= VOTE_BOUND and np.array_equal(v == 0, want == 0)
    # ---- equal to the golden
    for i in range(n):
        assert np.array_equal(res["preds"][i].cpu().numpy(), g["%s/preds_%d" % (tag, i)])
        assert np.array_equal(res["error"][i].cpu().numpy(), g["%s/error_%d" % (tag, i)])
    assert np.array_equal(tester.full_confusion, g[tag + "/conf_full"])
    assert np.array_equal(res["confusion"], g[tag + "/plot_conf"])
    assert np.array_equal(res["IoUs"], g[tag + "/iou_full"])
    assert len(tester.sub_IoUs) == 2
    for k, name in enumerate(("sub_checkpoint", "sub_end")):
        assert np.array_equal(tester.sub_confusions[k], g["%s/iou_in_%s" % (tag, name)])
        assert np.array_equal(tester.sub_IoUs[k], g["%s/iou_%s" % (tag, name)])
    assert np.array_equal(tester.val_proportions, g[tag + "/val_proportions"])
    lines = out.split("\n")
    want_lines = [str(s) for s in g[tag + "/lines"]]
    assert [l for l in lines if " | " in l] == want_lines
    dashes = '-' * len(want_lines[2])
    k = lines.index(want_lines[2])
    assert lines[k - 1] == dashes and lines[k + 1] == dashes and lines[k - 2] == 'Confusion on full clouds'
    assert [l for l in lines if l.startswith('Test epoch')] == [l for l in str(g[tag + "/stdout"]).split("\n") if l.startswith('Test epoch')]
    assert 'Reproject Vote #1' in lines and lines.count('Confusion on sub clouds') == 2
    # ---- the files
    path = res["path"]
    assert path == os.path.join(str(tmp_path), 'test', 'PseudoLabel' if tag == "A" else 'WeakLabel', 'Log_g21_' + tag)
    kept = [i for i, v in enumerate(lv) if v not in ign]
    for i in range(n):
        name = "cloud_%d.ply" % i
        for kind in ("predictions", "potentials"):
            with open(os.path.join(GOLDEN, "test_run", tag, kind, name), "rb") as f:
                assert f.read() == open(os.path.join(path, kind, name), "rb").read(), (kind, name)
        data = open(os.path.join(path, "probs", name), "rb").read()
        assert data.startswith(str(g["%s/probs_header_%d" % (tag, i)]).encode())          # the field layout
        back = read_ply(os.path.join(path, "probs", name))
        assert list(back.dtype.names) == [str(s) for s in g["%s/probs_fields_%d" % (tag, i)]]
        want = ref.kernel_outputs(get("votes_end")[i], get("proj")[i], kept, lv)[0]
        cols = np.stack([back[f] for f in back.dtype.names[3:]], axis=1)
        assert cols.dtype == np.float64 and np.abs(cols - want).max() <= VOTE_BOUND
        assert np.array_equal(cols, res["probs"][i].cpu().numpy().astype(np.float64))
    suffix = "G21_validation_conf.txt"
    assert np.array_equal(np.loadtxt(os.path.join(path, "predictions", suffix), dtype=np.int64), g[tag + "/plot_conf"])
    extra = sorted(f for f in os.listdir(path) if f.endswith(".npz"))
    if tag == "B":
        assert extra == ["probs.npz", "pseudo.npz"]
        with np.load(os.path.join(path, "pseudo.npz"), allow_pickle=False) as z:
            assert z.files == ["cloud_0.ply"] and np.array_equal(z["cloud_0.ply"], np.argmax(get("votes_end")[0], axis=1))
        with np.load(os.path.join(path, "probs.npz"), allow_pickle=False) as z:
            assert np.array_equal(z["cloud_0.ply"], tester.votes.probs[0].cpu().numpy())
    else:
        assert extra == []


def test_replay_that_does_not_end_raises(gpu, tmp_path):
    from weasal_amd import testrun
    g = golden("g21_test_run.npz")
    with pytest.raises(RuntimeError, match=r"after 3 test epochs \(minimum potentials: 0.300, 0.700, 1.200\)"):
        _replay(g, "A", gpu, tmp_path, testrun.ModelTester, max_test_epochs=3)


# ---------------------------------------------------------------------------------------------------------------------
# active learning: a pass over the training clouds that writes nothing
# ---------------------------------------------------------------------------------------------------------------------
def test_active_learning_points(gpu, tmp_path):
    from weasal_amd import tester as wt, testrun
    g = golden("g21_test_run.npz")
    used = [np.arange(0, 40, 3), np.array([5, 5, 17])]
    t, got, _, _ = _replay(g, "A", gpu, tmp_path, testrun.ModelTester, set_name="training", active_learning=True, used_ids=used)
    want = wt.active_learning_selection(t.votes, [0.1 * k for k in range(9)], used, 7)
    assert len(got) == 2 and all(np.array_equal(a, b) for a, b in zip(got, want))
    assert all(len(a) == len(u) + 7 and a.dtype == np.int64 for a, u in zip(got, used))
    assert os.listdir(str(tmp_path)) == [] and t.test_epochs == 4 and t.checkpoints == 2 and t._sync_count == 4
    assert t.sub_IoUs == []


def test_active_learning_anchors(gpu, tmp_path):
    import active_ref
    from weasal_amd import active, testrun
    g = golden("g21_test_run.npz")
    ptr, idx, labels = active_ref.synthetic_anchors(4, 150, 20, 4, lo=3, hi=30)
    sets = [types.SimpleNamespace(ptr=_dev(gpu, ptr), idx=_dev(gpu, idx), lb=labels)]
    used = [np.arange(6)]
    t, got, _, _ = _replay(g, "B", gpu, tmp_path, testrun.ModelTesterWL, set_name="training", active_learning=True, anchor_sets=sets,
                           used_anchors=used, added_labels=5)
    new = active.select_anchors(t.votes, 0, sets[0].ptr, sets[0].idx, labels, used[0], 5).cpu().numpy()
    assert len(got) == 1 and np.array_equal(got[0], np.append(used[0], new)) and len(got[0]) == 11
    assert os.listdir(str(tmp_path)) == []


# ---------------------------------------------------------------------------------------------------------------------
# a real run: two small tiles, the 16-feature network, a checkpoint of loop.ModelTrainer
# ---------------------------------------------------------------------------------------------------------------------
ONE_SPHERE = 1
NAMES = {k: "class %d" % k for k in range(9)}


def _config(saving_path):
    from weasal_amd import config as wcfg, synthetic
    cfg = wcfg.Vaihingen3DPLConfig()
    cfg.in_radius, cfg.in_features_dim, cfg.dropout = synthetic.WORKLOADS["vaihingen"]["radius"], 3, 0.0
    cfg.first_features_dim, cfg.num_classes, cfg.dataset_task = 16, 9, 'cloud_segmentation'
    cfg.max_epoch, cfg.epoch_steps, cfg.checkpoint_gap, cfg.lr_decays = 1, 1, 1, {0: 0.5}
    cfg.contrast_start, cfg.contrast_thd = 1, 10
    cfg.validation_size = 4
    cfg.saving, cfg.saving_path = saving_path is not None, saving_path
    return cfg


@pytest.fixture(scope="module")
def real(gpu, tmp_path_factory):
    """tiles on disk (10 m and 8 m across: a 4 m sphere covers most of one, so a few spheres lift every potential above
    0.5), a one-step training run that leaves current_chkp.tar, and the pieces of a test run"""
    from weasal_amd import pyramid, synthetic, testrun, validation
    from weasal_amd.architectures import KPFCNN
    from weasal_amd.loop import ModelTrainer
    from weasal_amd.ply import write_ply
    from weasal_amd.sampler import SphereSampler
    root = tmp_path_factory.mktemp("tiles")
    rs = np.random.RandomState(8)
    names, files = ["tile_a", "tile_b"], []
    for name, half in zip(names, (5.0, 4.0)):
        raw = (rs.uniform(-1, 1, size=(int(44 * half * half * 4), 3)) * np.array([half, half, 2.0])).astype(np.float32)
        files.append(str(root / (name + ".ply")))
        assert write_ply(files[-1], [raw, rs.randint(0, 9, size=raw.shape[0]).astype(np.int32)], ['x', 'y', 'z', 'class'])
    log = str(tmp_path_factory.mktemp("train") / "Log_real")
    cfg = _config(log)
    ts, clouds = testrun.TestSet.from_cache(str(root), names, files, cfg.first_subsampling_dl, gpu, np.arange(9), [], NAMES,
                                            set='validation', name='Synthetic', coord_offset=np.array([[10.0, 20.0, 30.0]], np.float32))
    wl = synthetic.WORKLOADS["vaihingen"]

    def network():
        np.random.seed(3)
        torch.manual_seed(3)
        return KPFCNN(cfg, np.arange(9), []).to(gpu)

    net = network().train()
    train_sampler = SphereSampler(cfg, clouds, label_values=np.arange(9), seed=11, max_spheres=16, batch_limit=ONE_SPHERE)
    orient = np.random.RandomState(1)
    ModelTrainer(net, cfg, device=gpu).train(net, lambda epoch: (pyramid.build_batch(cfg, *train_sampler.sample()[:4], wl["limits"], rng=orient)
                                                                 for _ in range(cfg.epoch_steps)))
    chkp = os.path.join(log, "checkpoints", "current_chkp.tar")
    assert os.path.exists(chkp)

    def run(out_root, **kw):
        fresh = network()
        tester = testrun.ModelTester(fresh, cfg, chkp_path=chkp, device=gpu)
        assert tester.epoch == 1 and not fresh.training
        for (k, a), (_, b) in zip(fresh.state_dict().items(), net.state_dict().items()):
            assert torch.equal(a, b), k
        s = SphereSampler(cfg, clouds, set='validation', label_values=np.arange(9), seed=5, max_spheres=16, batch_limit=ONE_SPHERE)
        rng = np.random.RandomState(2)

        def batches(epoch):
            for _ in range(cfg.validation_size):
                item = s.sample()
                yield pyramid.build_batch(cfg, *item[:4], wl["limits"], rng=rng, for_training=False), validation.fields_from_sampler(s, item)
        kw.setdefault("max_test_epochs", 40)
        res = tester.cloud_segmentation_test(fresh, s, batches, ts, num_votes=0, root=str(out_root), **kw)
        return tester, s, res
    return dict(run=run, ts=ts, clouds=clouds, cfg=cfg, names=names)


def _tree(path):
    return {os.path.relpath(os.path.join(d, f), path): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(path) for f in fs}


def test_real_run_ends_and_writes_what_it_computed(real, tmp_path):
    from weasal_amd.ply import read_ply
    tester, sampler, res = real["run"](tmp_path / "one")
    ts = real["ts"]
    print("test epochs", tester.test_epochs, "minima", ["%.3f" % v for v in tester.minima], "sampler reads", sampler._sync_count)
    assert tester.minima[-1] > 0.5 and all(v <= 0.5 for v in tester.minima[:-1]) and tester.checkpoints == 1
    assert tester._sync_count == tester.test_epochs + 1 + 1
    assert sampler._sync_count == tester.test_epochs * real["cfg"].validation_size         # the sampler's own read per batch
    files = _tree(res["path"])
    assert sorted(files) == sorted([os.path.join(k, n + ".ply") for k in ("predictions", "probs", "potentials") for n in real["names"]]
                                   + [os.path.join("predictions", "Synthetic_validation_conf.txt")])
    total = np.zeros((9, 9), np.int64)
    for i, name in enumerate(real["names"]):
        for kind in ("predictions", "probs", "potentials"):
            assert len(read_ply(os.path.join(res["path"], kind, name + ".ply"))) > 0
        pred = read_ply(os.path.join(res["path"], "predictions", name + ".ply"))
        assert pred.dtype.names == ('x', 'y', 'z', 'preds', 'targets', 'error')
        votes = tester.votes.probs[i].cpu().numpy()
        proj, targets = ts.proj[i].cpu().numpy(), ts.labels[i].cpu().numpy()
        probs, preds, error, conf = ref.cloud_outputs(votes, proj, np.arange(9), [], targets)
        assert np.array_equal(pred['preds'], preds) and np.array_equal(pred['error'], error) and np.array_equal(pred['targets'], targets)
        assert 0 < int((votes.sum(axis=1) > 0).sum()) and len(np.unique(preds)) > 1
        back = read_ply(os.path.join(res["path"], "probs", name + ".ply"))
        assert back.dtype.names[3:] == tuple("class_%d" % k for k in range(9))
        assert np.array_equal(np.stack([back[f] for f in back.dtype.names[3:]], axis=1), probs.astype(np.float64))
        pts = ts.points(i)
        assert pts.dtype == np.float32 and np.array_equal(pred['x'], pts[:, 0]) and np.array_equal(back['z'], pts[:, 2])
        total += conf
    assert np.array_equal(res["confusion"], total)
    assert np.array_equal(np.loadtxt(os.path.join(res["path"], "predictions", "Synthetic_validation_conf.txt"), dtype=np.int64), total)
    # a second run under the same seeds: the same bytes
    _, _, res2 = real["run"](tmp_path / "two")
    assert _tree(res2["path"]) == files


def test_real_run_that_cannot_end_in_one_epoch_raises(real, tmp_path):
    with pytest.raises(RuntimeError, match="after 1 test epochs"):
        real["run"](tmp_path, max_test_epochs=1)
