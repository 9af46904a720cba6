"""The price of batch normalisation over the points in the whole training step: train_step of DALESPLConfig on the synthetic
DALES batches (prebuilt: no pyramid work in the timed window) in 'reference' mode (the identity of models/blocks.py:453-463,
every block one fused call) against 'points' mode (raw products + ops.batch_norm_act, every fused route declined).  The two
networks alternate step by step after warm-up; per step a HIP-event interval and the library's launch count
(ws_launch_count).  Medians and the min-max spread.  No pass/fail threshold is attached."""
import json, os, sys
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from weasal_amd import _lib, config as wcfg, pyramid, synthetic
from weasal_amd.architectures import KPFCNN
from weasal_amd.trainer import make_optimizer, train_step

WARMUP, REPS = 4, 12
dev = torch.device("cuda:0")
lib = _lib.lib()
wl = synthetic.WORKLOADS["dales"]
nets = {}
for mode in ("reference", "points"):
    cfg = wcfg.DALESPLConfig()
    if mode == "points":
        cfg.batch_norm_mode = "points"
    torch.manual_seed(0); np.random.seed(0)
    net = KPFCNN(cfg, np.arange(9), []).to(dev).train()
    nets[mode] = (net, make_optimizer(net, cfg), cfg)
batches = []
for s in range(2):
    pts, feats, labels, lens = synthetic.make_inputs(s, wl["spheres"], wl["points"], wl["radius"], nets["reference"][2].in_features_dim)
    batches.append(pyramid.build_batch(nets["reference"][2], torch.from_numpy(pts).to(dev), torch.from_numpy(feats).to(dev),
                                       torch.from_numpy(labels).to(dev), lens, wl["limits"]))
times = {m: [] for m in nets}
launches = {}
for it in range(WARMUP + REPS):
    for mode, (net, opt, cfg) in nets.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        before = lib.ws_launch_count()
        e0.record(); train_step(net, opt, batches[it % 2], cfg); e1.record()
        torch.cuda.synchronize()
        launches[mode] = int(lib.ws_launch_count() - before)
        if it >= WARMUP:
            times[mode].append(e0.elapsed_time(e1))
res = {m: dict(ms_per_step_median=float(np.median(t)), ms_min=float(min(t)), ms_max=float(max(t)), library_launches_per_step=launches[m])
       for m, t in times.items()}
res["rows_level0"] = int(batches[0].points[0].shape[0])
os.makedirs(os.path.join(REPO, "bench_outputs"), exist_ok=True)
json.dump(res, open(os.path.join(REPO, "bench_outputs", "bn_step_ab.json"), "w"), indent=1)
print(json.dumps(res))
