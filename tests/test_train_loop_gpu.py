"""GPU: weasal_amd.loop.ModelTrainer / ModelTrainerWL on two small synthetic tiles (the ones of
test_sampler_gpu.test_sampler_feeds_the_prefetcher_the_votes_and_a_training_step), the Vaihingen-sized networks at 16 first
features, max_epoch 2, epoch_steps 3, checkpoint_gap 1, lr_decays {0: 0.5}.

The reference for the log is a second run under the same seeds that calls trainer.train_step by hand and reads
`net.output_loss.item()` and `net.accuracy(...)` after every step, as the reference's loop does: the ring's loss words must
be those bits, `correct` that integer, and the file's columns the same three decimals.  The contrastive term joins in epoch
1 (contrast_start = 1): the hand run sees only loss = fl(fl(out + reg) + contrast), so the `extra` column is held to
|extra - (loss - out - reg)| <= 2^-22 |loss| -- two roundings of the sum and one of each difference, each at most half an
ulp of a number no larger than |loss| (all terms are positive)."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# a point budget of 1: every batch is one sphere of about 2 000 points (the stop rule of the sampler).  The smallest batch
# that still trains, and below the 4 096 rows from which the input layer's product takes its streaming form, which asks for
# more LDS than a launch gets when the layer has fewer than 32 output columns (first_features_dim < 64).
ONE_SPHERE = 1


def _tiles(gpu, dl, colours=False):
    from weasal_amd import ops
    rs = np.random.RandomState(8)
    clouds = []
    for half in (10.0, 8.0):
        raw = (rs.uniform(-1, 1, size=(int(44 * half * half * 4), 3)) * np.array([half, half, 2.0])).astype(np.float32)
        P = torch.from_numpy(raw).to(gpu)
        sub = ops.grid_subsample(P, np.array([P.shape[0]], np.int32), dl)[0]
        cloud = (sub, torch.from_numpy(rs.randint(0, 9, size=sub.shape[0]).astype(np.int32)).to(gpu))
        if colours:
            cloud += (torch.from_numpy(rs.uniform(0, 1, size=(sub.shape[0], 1)).astype(np.float32)).to(gpu),)
        clouds.append(cloud)
    return clouds


def _pl_config(saving_path):
    from weasal_amd import config as wcfg, synthetic
    cfg = wcfg.Vaihingen3DPLConfig()
    cfg.in_radius, cfg.in_features_dim, cfg.dropout = synthetic.WORKLOADS["vaihingen"]["radius"], 3, 0.0
    cfg.first_features_dim, cfg.num_classes, cfg.dataset_task = 16, 9, 'cloud_segmentation'
    cfg.max_epoch, cfg.epoch_steps, cfg.checkpoint_gap, cfg.lr_decays = 2, 3, 1, {0: 0.5}
    cfg.contrast_start, cfg.contrast_thd = 1, 10
    cfg.saving, cfg.saving_path = saving_path is not None, saving_path
    return cfg


def _pl_setup(gpu, cfg, clouds):
    """-> (net, batches): everything that draws is seeded here, so two set-ups serve the same batches to the same network"""
    from weasal_amd import pyramid, synthetic
    from weasal_amd.architectures import KPFCNN
    from weasal_amd.sampler import SphereSampler
    wl = synthetic.WORKLOADS["vaihingen"]
    s = SphereSampler(cfg, clouds, label_values=np.arange(9), seed=11, max_spheres=16, batch_limit=ONE_SPHERE)
    orient = np.random.RandomState(1)
    np.random.seed(3)
    torch.manual_seed(3)
    net = KPFCNN(cfg, np.arange(9), []).to(gpu).train()

    def batches(epoch):
        for _ in range(cfg.epoch_steps):
            yield pyramid.build_batch(cfg, *s.sample()[:4], wl["limits"], rng=orient)
    return net, batches


def _read_log(path):
    with open(path) as f:
        lines = f.read().split("\n")
    assert lines[-1] == ""
    return lines[0], [l.split(" ") for l in lines[1:-1]]


@pytest.fixture(scope="module")
def clouds(gpu):
    from weasal_amd import config as wcfg
    return _tiles(gpu, wcfg.Vaihingen3DPLConfig.first_subsampling_dl)


@pytest.fixture(scope="module")
def pl_run(gpu, clouds, tmp_path_factory):
    """the run under test and the hand-run twin"""
    from weasal_amd.loop import ModelTrainer
    from weasal_amd.trainer import make_optimizer, train_step
    path = str(tmp_path_factory.mktemp("pl") / "log")
    cfg = _pl_config(path)
    net, batches = _pl_setup(gpu, cfg, clouds)
    trainer = ModelTrainer(net, cfg, device=gpu)
    assert os.path.exists(os.path.join(path, "parameters.txt"))
    trainer.train(net, batches, header_note="12 of 34")
    # ---- by hand, the reference's way: a read after every step
    cfg2 = _pl_config(None)
    twin, batches2 = _pl_setup(gpu, cfg2, clouds)
    opt = make_optimizer(twin, cfg2)
    hand = []
    for epoch in range(cfg2.max_epoch):
        for batch in batches2(epoch):
            loss, out = train_step(twin, opt, batch, cfg2, epoch=epoch)
            out_loss = twin.output_loss.item()
            acc = twin.accuracy(out, batch.labels)
            hand.append((epoch, out_loss, float(twin.reg_loss), acc, int(out.shape[0]), loss.item()))
        for g in opt.param_groups:
            g['lr'] *= cfg2.lr_decays.get(epoch, 1.0)
    return dict(path=path, cfg=cfg, net=net, trainer=trainer, hand=hand, twin=twin, twin_opt=opt)


def test_log_file_equals_the_hand_run(pl_run):
    header, lines = _read_log(os.path.join(pl_run["path"], "training_iteration0.txt"))
    assert header == "epochs steps out_loss offset_loss train_accuracy time \tground truth labels: 12 of 34"
    assert [l[:2] for l in lines] == [["0", "0"], ["0", "1"], ["0", "2"], ["1", "0"], ["1", "1"], ["1", "2"]]
    times = [float(l[5]) for l in lines]
    assert all(len(l) == 6 for l in lines) and all(b >= a for a, b in zip(times, times[1:])) and times[0] >= 0
    for l, (_, out_loss, reg, acc, _, _) in zip(lines, pl_run["hand"]):
        print(" ".join(l), "| by hand: %.6f %.6f %.6f" % (out_loss, reg, acc))
        assert l[2:5] == ["%.3f" % out_loss, "%.3f" % reg, "%.3f" % acc]
        assert len(l[5].split(".")[1]) == 3


def test_ring_values_are_the_hand_runs_bits(pl_run):
    t = pl_run["trainer"]
    assert t.log.host_reads == 2 and t.log.grown == 0 and t.log.capacity == 3
    recs = np.concatenate(t.records)
    rows = [r for epoch in t.rows for r in epoch]
    assert len(recs) == len(rows) == len(pl_run["hand"]) == 6
    for rec, row, (epoch, out_loss, reg, acc, n, loss) in zip(recs, rows, pl_run["hand"]):
        assert np.float32(out_loss).tobytes() == rec['out_loss'].tobytes()
        assert np.float32(reg).tobytes() == rec['reg_loss'].tobytes()
        assert int(rec['correct']) == round(acc * n) and row[3] == int(rec['correct']) / n == acc
        assert 0 < int(rec['correct']) < n
        if epoch == 0:
            assert rec['extra'].tobytes() == np.float32(0).tobytes()
        else:
            implied = loss - out_loss - reg
            print("contrastive term %.7f, implied by the hand run's total %.7f" % (rec['extra'], implied))
            assert rec['extra'] > 0 and abs(float(rec['extra']) - implied) <= 2.0 ** -22 * abs(loss)
    assert "contrast_loss" not in vars(pl_run["net"])                                   # train() took its wrapper off again


def test_learning_rates_and_the_networks_agree(pl_run):
    cfg, t = pl_run["cfg"], pl_run["trainer"]
    assert [g['lr'] for g in t.optimizer.param_groups] == [cfg.learning_rate * 0.5, cfg.learning_rate * cfg.deform_lr_factor * 0.5]
    assert t.epoch == 2 and t.step == 3
    for (k, a), (_, b) in zip(pl_run["net"].state_dict().items(), pl_run["twin"].state_dict().items()):
        assert torch.equal(a, b), k


def test_checkpoints_restore_and_finetune(pl_run, gpu, clouds):
    from weasal_amd.loop import ModelTrainer
    path, cfg, t = pl_run["path"], pl_run["cfg"], pl_run["trainer"]
    chk = os.path.join(path, "checkpoints")
    assert sorted(os.listdir(chk)) == ["chkp_0002_0.tar", "chkp_0003_0.tar", "current_chkp.tar"]
    assert not os.path.exists(os.path.join(path, "running_PID.txt"))                    # removed after the last epoch
    current = torch.load(os.path.join(chk, "current_chkp.tar"), weights_only=True)
    for name, epoch in (("current_chkp.tar", 2), ("chkp_0002_0.tar", 1), ("chkp_0003_0.tar", 2)):
        c = torch.load(os.path.join(chk, name), weights_only=True)
        assert sorted(c) == ["epoch", "model_state_dict", "optimizer_state_dict", "saving_path"]
        assert c["epoch"] == epoch and c["saving_path"] == path
    for k, v in pl_run["net"].state_dict().items():
        assert torch.equal(current["model_state_dict"][k].to(v.device), v), k
    cfg2 = _pl_config(None)
    fresh, _ = _pl_setup(gpu, cfg2, clouds)
    r = ModelTrainer(fresh, cfg2, chkp_path=os.path.join(chk, "current_chkp.tar"), device=gpu)
    assert r.epoch == 2 and [g['lr'] for g in r.optimizer.param_groups] == [g['lr'] for g in t.optimizer.param_groups]
    bufs = 0
    for p_new, p_old in zip(fresh.parameters(), pl_run["net"].parameters()):
        assert torch.equal(p_new, p_old)
        a, b = r.optimizer.state[p_new].get('momentum_buffer'), t.optimizer.state[p_old].get('momentum_buffer')
        assert (a is None) == (b is None)
        if a is not None:
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
            bufs += 1
    assert bufs > 10 and fresh.training
    fresh2, _ = _pl_setup(gpu, cfg2, clouds)
    f = ModelTrainer(fresh2, cfg2, chkp_path=os.path.join(chk, "chkp_0002_0.tar"), finetune=True, device=gpu)
    assert f.epoch == 0 and [g['lr'] for g in f.optimizer.param_groups] == [cfg.learning_rate, cfg.learning_rate * cfg.deform_lr_factor]
    assert not f.optimizer.state


def test_parameters_txt_loads_back_equal(pl_run):
    from weasal_amd import config as wcfg
    cfg = pl_run["cfg"]
    back = wcfg.Config().load(pl_run["path"])
    for key in ("dataset", "num_classes", "in_radius", "architecture", "first_features_dim", "learning_rate", "momentum", "lr_decays",
                "grad_clip_norm", "max_epoch", "epoch_steps", "checkpoint_gap", "contrast_start", "contrast_thd", "dropout",
                "num_layers", "deform_layers", "batch_num", "in_features_dim", "first_subsampling_dl"):
        assert getattr(back, key) == getattr(cfg, key), key


def test_kill_file_stops_the_run_after_epoch_0(gpu, clouds, tmp_path):
    from weasal_amd.loop import ModelTrainer
    path = str(tmp_path / "log")
    cfg = _pl_config(path)
    net, batches = _pl_setup(gpu, cfg, clouds)
    served = []

    def killing(epoch):
        if epoch == 1:
            os.remove(os.path.join(path, "running_PID.txt"))
        for b in batches(epoch):
            served.append(epoch)
            yield b
    t = ModelTrainer(net, cfg, device=gpu)
    t.train(net, killing)
    _, lines = _read_log(os.path.join(path, "training_iteration0.txt"))
    assert [l[:2] for l in lines] == [["0", "0"], ["0", "1"], ["0", "2"]]
    assert served == [0, 0, 0, 1] and t.epoch == 1 and t.log.host_reads == 1
    c = torch.load(os.path.join(path, "checkpoints", "current_chkp.tar"), weights_only=True)
    assert c["epoch"] == 1 and sorted(os.listdir(os.path.join(path, "checkpoints"))) == ["chkp_0002_0.tar", "current_chkp.tar"]


def test_rank_1_writes_nothing(gpu, clouds, tmp_path):
    from weasal_amd.loop import ModelTrainer
    cfg = _pl_config(str(tmp_path / "log"))
    cfg.max_epoch = 1
    net, batches = _pl_setup(gpu, cfg, clouds)
    t = ModelTrainer(net, cfg, device=gpu, rank=1)
    t.train(net, batches)
    assert os.listdir(str(tmp_path)) == [] and t.epoch == 1 and len(t.rows[0]) == 3 and t.log.host_reads == 1


def test_ring_grows_when_the_epoch_runs_longer(gpu, clouds):
    from weasal_amd.loop import ModelTrainer
    cfg = _pl_config(None)
    cfg.max_epoch = 1
    net, batches = _pl_setup(gpu, cfg, clouds)
    cfg.epoch_steps = 3                                     # the batches: three
    t = ModelTrainer(net, cfg, device=gpu)
    short = copy.copy(cfg)
    short.epoch_steps = 1                                   # the ring: one record, then two, then four
    t.train(net, batches, config=short)
    assert (t.log.capacity, t.log.grown, t.log.host_reads) == (4, 2, 1) and len(t.rows[0]) == 3
    assert all(np.isfinite(r[0]) and 0 < r[3] < 1 for r in t.rows[0])
    assert [r[4] for r in t.rows[0]] == sorted(r[4] for r in t.rows[0])


def test_step_log_on_the_device_peek_and_flush(gpu):
    """StepLog itself: peek() reads the newest finished step without counting as the epoch's read, flush() returns every row
    with the time of its event, and the console line of a run whose period is 0 shows finished steps only"""
    from weasal_amd.loop import StepLog
    log = StepLog(2, gpu)
    log.start()
    assert log.peek() is None and log.flush() == [] and log.host_reads == 0
    x = torch.eye(4, 9, device=gpu)
    lab = torch.tensor([0, 1, 5, 3], device=gpu)
    for i in range(3):
        assert log.record(x, lab, None, torch.full((1,), 1.5 + i, device=gpu), None, None) == i
    torch.cuda.synchronize()
    step, row = log.peek()
    assert step == 2 and row[:4] == (3.5, 0.0, 0.0, 0.75) and row[4] >= 0 and (log.peeks, log.host_reads) == (1, 0)
    rows = log.flush()
    assert [r[:4] for r in rows] == [(1.5 + i, 0.0, 0.0, 0.75) for i in range(3)] and rows[2] == row
    assert [r[4] for r in rows] == sorted(r[4] for r in rows) and (log.host_reads, log.grown, log.capacity) == (1, 1, 4)
    assert log.last_records['correct'].tolist() == [3, 3, 3] and log.peek() is None


def test_console_line_shows_finished_steps(gpu, clouds, capsys):
    from weasal_amd.loop import ModelTrainer
    cfg = _pl_config(None)
    cfg.max_epoch = 1
    net, batches = _pl_setup(gpu, cfg, clouds)
    t = ModelTrainer(net, cfg, device=gpu)
    t.console_every = 0.0

    def waiting(epoch):
        for b in batches(epoch):
            yield b
            torch.cuda.synchronize()          # (the test's own wait, outside the loop's code: every step has finished)
    t.train(net, waiting)
    import re
    out = [l for l in capsys.readouterr().out.split("\n") if l.startswith("e000-i")]
    for l in out:
        assert re.fullmatch(r"e000-i000[012] => L=\d\.\d{3} acc=[ \d]{3}% / t=\d+\.\d s \| al_iteration=0", l), l
    steps = [int(l[6:10]) for l in out]
    # after steps 1 and 2 the step before has surely finished; after step 0 the line shows only if the GPU already has
    assert len(out) in (2, 3) and steps == sorted(steps) and steps[-1] >= 1 and steps[-2] >= 0
    assert t.log.peeks == len(out) and t.log.host_reads == 1


# ---------------------------------------------------------------------------------------------------------------------
def _wl_setup(gpu, cfg, clouds):
    from weasal_amd import anchors, pyramid, synthetic
    from weasal_amd.architectures import KPFCNN_mprm
    from weasal_amd.sampler import SphereSampler
    wl = synthetic.WORKLOADS["vaihingen_wl"]
    s = SphereSampler(cfg, clouds, label_values=np.arange(9), seed=11, max_spheres=16, batch_limit=ONE_SPHERE)
    sets = []
    for c in clouds:
        a = anchors.anchors_with_points(c[0], c[1].to(torch.int64), anchors.get_anchors(c[0], cfg.sub_radius, 'reduced'), cfg.sub_radius,
                                        cfg.num_classes)
        sets.append(anchors.update_anchors(a, c[0], cfg.sub_radius))
    s.set_anchors(sets)
    orient = np.random.RandomState(1)
    np.random.seed(3)
    torch.manual_seed(3)
    net = KPFCNN_mprm(cfg, np.arange(9), []).to(gpu).train()

    def batches(epoch):
        for i in range(cfg.epoch_steps):
            out = s.sample()
            batch = pyramid.build_batch(cfg, *out[:4], wl["limits"], rng=orient)
            if i == 1:
                s.last_centres = s.last_centres + 500.0       # no anchor within reach: no region survives the cut
            batch.region, batch.region_lb = s.cut_regions(), None
            batch.cloud_lb = batch.region.cloud_lb
            batch.center_pts = torch.from_numpy(s.last_centres.astype(np.float32)).to(gpu)
            yield batch
    return net, batches


def test_weak_label_run_skips_the_batch_without_regions(gpu, tmp_path):
    from weasal_amd import config as wcfg, synthetic
    from weasal_amd.loop import ModelTrainerWL
    from weasal_amd.trainer import make_optimizer, train_step_weak

    def config(path):
        cfg = wcfg.Vaihingen3DWLConfig()
        cfg.in_radius, cfg.sub_radius = synthetic.WORKLOADS["vaihingen_wl"]["radius"], 1.0
        cfg.first_features_dim, cfg.dataset_task = 16, 'cloud_segmentation'
        cfg.max_epoch, cfg.epoch_steps, cfg.checkpoint_gap = 1, 3, 1
        cfg.saving, cfg.saving_path = path is not None, path
        return cfg
    clouds = _tiles(gpu, wcfg.Vaihingen3DWLConfig.first_subsampling_dl, colours=True)
    path = str(tmp_path / "log")
    cfg = config(path)
    net, batches = _wl_setup(gpu, cfg, clouds)
    t = ModelTrainerWL(net, cfg, device=gpu)
    t.train(net, batches, header_note="40 (30)")
    header, lines = _read_log(os.path.join(path, "training_iteration0.txt"))
    assert header == "epochs steps out_loss offset_loss train_accuracy time \tweak labels (initial): 40 (30)"
    assert [l[:2] for l in lines] == [["0", "0"], ["0", "1"]]
    assert t.step == 2 and t.log.host_reads == 1 and len(t.records[0]) == 2
    assert [g['lr'] for g in t.optimizer.param_groups] == [cfg.learning_rate, cfg.learning_rate * cfg.deform_lr_factor]   # no decay at epoch 0
    # by hand
    cfg2 = config(None)
    twin, batches2 = _wl_setup(gpu, cfg2, clouds)
    opt = make_optimizer(twin, cfg2)
    hand = []
    for batch in batches2(0):
        loss, out = train_step_weak(twin, opt, batch, cfg2)
        if loss is None:
            hand.append(None)
            continue
        hand.append((twin.output_loss.item(), twin.grad_norm.item(), twin.accuracy(out[0], batch.labels), int(out[0].shape[0])))
    assert [h is None for h in hand] == [False, True, False]
    for rec, l, h in zip(t.records[0], lines, [h for h in hand if h is not None]):
        print(" ".join(l), "| by hand: loss %.6f norm %.6f acc %.6f" % h[:3])
        assert np.float32(h[0]).tobytes() == rec['out_loss'].tobytes()
        assert np.float32(h[1]).tobytes() == rec['extra'].tobytes() and h[1] > 0
        assert int(rec['correct']) == round(h[2] * h[3]) and rec['reg_loss'] == 0
        assert l[2:5] == ["%.3f" % h[0], "0.000", "%.3f" % h[2]]
