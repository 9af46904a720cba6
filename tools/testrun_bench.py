"""The end of a test run and one test epoch, each against what the code before weasal_amd.testrun offered, in one process.

(a) ws_test_outputs on a DALES-sized tile -- 12 M full-resolution points re-projected on a 3 M point sub-cloud, 9 vote
    columns of 10 label values ([0..8, 10], 10 ignored) -- against the earlier route to the same arrays:
    VoteAccumulator.predictions (the `p[proj]` copy for the voted mask, ws_project_confusion and the framework passes of the
    ignored-label rule), a second `p[proj]` gather for the probability rows, the column insertion and the error map in torch.
    Both produce proj_probs [m, 10] float32, preds int32, error int8 and the confusion; they are compared before timing.
    Bytes the algorithm needs (from shapes): proj 4 m, targets 4 m, one vote row per point 4 c m (gathered; at most the
    whole vote buffer is distinct), written 4 c_all m + 4 m + m.  Achieved bandwidth = those bytes over the event time.
(b) one test epoch of testrun.ModelTester (forward under no_grad, update_batch, the one read of the minimum potential)
    against a bare loop of forward + update_batch over the same prebuilt batches that ends in a synchronise: Vaihingen
    KP-FCNN, one 4 m sphere per batch.

After warm-up the two forms of each part alternate; HIP events for (a), wall time around work that ends in a synchronise
or a blocking read for (b).  Medians, minima and maxima; no pass/fail threshold.  `--part a` / `--part b` runs one part."""
import json, os, sys, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from weasal_amd import tester, testrun, validation

WARMUP, REPS = 3, 20
dev = torch.device("cuda:0")
stat = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
part = sys.argv[sys.argv.index("--part") + 1] if "--part" in sys.argv else "ab"
res = dict(warmup=WARMUP, reps=REPS, cpu_threads=os.environ.get("OMP_NUM_THREADS"))

if "a" in part:
    M, N_SUB, LV, IGN = 12_000_000, 3_000_000, list(range(9)) + [10], [10]
    g = torch.Generator(device=dev).manual_seed(0)
    tables = testrun.LabelTables(LV, IGN, dev)
    c, c_all = tables.c, tables.c_all
    votes = tester.VoteAccumulator([N_SUB], c, dev)
    votes.probs[0].copy_(torch.rand((N_SUB, c), device=dev, generator=g) * 0.3)
    votes.probs[0][torch.rand(N_SUB, device=dev, generator=g) < 0.05] = 0          # sub-points nobody voted on
    # a full-resolution tile lists its points in file order, the sub-cloud in hash-map order: a random gather
    proj = torch.randint(0, N_SUB, (M,), device=dev, generator=g, dtype=torch.int32)
    targets = tables.values[torch.randint(0, c_all, (M,), device=dev, generator=g)].contiguous()
    kept = tables.col_of.long()
    status = testrun.new_status(dev)

    def new():
        conf = torch.zeros((c_all, c_all), dtype=torch.int64, device=dev)
        probs, preds, error = testrun.outputs(votes.probs[0], tables, status, proj=proj, targets=targets, confusion=conf, probs=True,
                                              error=True)
        return probs, preds, error, conf

    def old():
        preds, conf = votes.predictions(0, proj=proj, labels=targets, label_values=LV, ignored_labels=IGN)
        rows = votes.probs[0][proj.long()]
        probs = torch.zeros((M, c_all), dtype=torch.float32, device=dev)
        probs[:, kept] = rows
        error = (preds != targets).to(torch.int8)
        return probs, preds, error, conf

    a, b = new(), old()
    same = dict(proj_probs=bool(torch.equal(a[0], b[0])), preds=bool(torch.equal(a[1], b[1])), error=bool(torch.equal(a[2], b[2])),
                confusion=bool(torch.equal(a[3][kept][:, kept], b[3])), status=status.cpu().tolist())
    del a, b
    times = {"ws_test_outputs": [], "earlier_route": []}
    for it in range(WARMUP + REPS):
        for name, fn in (("ws_test_outputs", new), ("earlier_route", old)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(); out = fn(); e1.record()
            torch.cuda.synchronize()
            del out
            if it >= WARMUP:
                times[name].append(e0.elapsed_time(e1))
    needed = M * (4 + 4 + 4 * c + 4 * c_all + 4 + 1)
    res["outputs"] = dict(full_points=M, sub_points=N_SUB, vote_columns=c, label_values=c_all, equal_to_earlier_route=same,
                          bytes_needed=needed, event_ms={k: stat(v) for k, v in times.items()},
                          achieved_GBps={k: needed / (np.median(v) * 1e-3) / 1e9 for k, v in times.items()},
                          speedup_median=float(np.median(times["earlier_route"]) / np.median(times["ws_test_outputs"])))

if "b" in part:
    import types
    from weasal_amd import config as wcfg, ops, pyramid, synthetic
    from weasal_amd.architectures import KPFCNN
    from weasal_amd.sampler import SphereSampler
    wl = synthetic.WORKLOADS["vaihingen"]
    cfg = wcfg.Vaihingen3DPLConfig()
    cfg.in_radius, cfg.in_features_dim, cfg.dropout, cfg.num_classes, cfg.saving = wl["radius"], 3, 0.0, 9, False
    BATCHES = 16
    cfg.validation_size = BATCHES
    rs = np.random.RandomState(8)
    clouds = []
    for half in (20.0, 16.0):
        raw = (rs.uniform(-1, 1, size=(int(44 * half * half * 4), 3)) * np.array([half, half, 2.0])).astype(np.float32)
        P = torch.from_numpy(raw).to(dev)
        sub = ops.grid_subsample(P, np.array([P.shape[0]], np.int32), cfg.first_subsampling_dl)[0]
        clouds.append((sub, torch.from_numpy(rs.randint(0, 9, size=sub.shape[0]).astype(np.int32)).to(dev)))
    s = SphereSampler(cfg, clouds, set='validation', label_values=np.arange(9), seed=5, max_spheres=16, batch_limit=1)
    np.random.seed(3); torch.manual_seed(3)
    net = KPFCNN(cfg, np.arange(9), []).to(dev).eval()
    orient = np.random.RandomState(2)
    items = []
    for _ in range(BATCHES):
        item = s.sample()
        items.append((pyramid.build_batch(cfg, *item[:4], wl["limits"], rng=orient, for_training=False), validation.fields_from_sampler(s, item)))
    ts = testrun.TestSet(["a", "b"], ["a.ply", "b.ply"], np.arange(9), [], {k: str(k) for k in range(9)}, 'test',
                         [None, None])
    mt = testrun.ModelTester(net, cfg, device=dev)
    sizes = [int(p.shape[0]) for p in s.sub_points]

    def epoch_tester():
        out = mt.cloud_segmentation_test(net, s, lambda e: items, ts, num_votes=-1, max_test_epochs=1)     # leaves after one epoch
        assert out is None and mt.test_epochs == 1 and mt._sync_count == 1

    bare_votes = tester.VoteAccumulator(sizes, 9, dev)

    def epoch_bare():
        with torch.no_grad():
            for batch, f in items:
                bare_votes.update_batch(net(batch, cfg), f["lengths"], f["input_inds"], f["cloud_inds"], points0=f["points"],
                                        radius_mask=0.7 * cfg.in_radius)
        torch.cuda.synchronize()

    import contextlib, io
    times = {"model_tester": [], "bare_loop": []}
    for it in range(WARMUP + REPS):
        for name, fn in (("model_tester", epoch_tester), ("bare_loop", epoch_bare)):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                fn()
            if it >= WARMUP:
                times[name].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    res["epoch"] = dict(batches=BATCHES, rows_per_batch=[int(b.points[0].shape[0]) for b, _ in items], wall_ms={k: stat(v) for k, v in times.items()},
                        overhead_ms_per_epoch=med["model_tester"] - med["bare_loop"],
                        overhead_percent=100 * (med["model_tester"] - med["bare_loop"]) / med["bare_loop"])
print(json.dumps(res))
