"""What folding the evaluation-mode batch normalisation buys in the forward-only pass: DALESPLConfig with
`batch_norm_mode = 'points'` on the synthetic DALES batches of tools/bn_step_ab.py (prebuilt: no pyramid work in the timed
window), under net.eval() and torch.no_grad() -- the pass of validation.run_epoch, testrun.ModelTester and refine.  Three arms
alternate forward by forward after warm-up:

    fold_on     every BatchNormBlock folded into its product (ops.bn_fold, one fold per forward), the fused routes taken
    fold_off    WEASAL_BN_FOLD=0: raw products followed by ws_bn_fwd's evaluation launch, operator by operator
    reference   the same network in reference mode (BatchNormBlock the identity): the yardstick for time, since the folded
                forward runs the same kernels plus the fold

Per forward a HIP-event interval and the library's launch count (ws_launch_count; the fold's launches are reported apart).
Mean, median and max - min per arm.  --arms selects arms (a build without the fold runs `fold_off,reference`: its 'points'
evaluation forward is the fold_off arm); --tag names the run in the output.  No pass/fail threshold is attached."""
import argparse, json, os, sys
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from weasal_amd import _lib, config as wcfg, ops, pyramid, synthetic
from weasal_amd.architectures import KPFCNN

ap = argparse.ArgumentParser()
ap.add_argument("--arms", default="fold_on,fold_off,reference")
ap.add_argument("--warmup", type=int, default=4)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--tag", default="")
args = ap.parse_args()
arms = args.arms.split(",")
dev = torch.device("cuda:0")
lib = _lib.lib()
wl = synthetic.WORKLOADS["dales"]
nets = {}
for mode in ("reference", "points"):
    cfg = wcfg.DALESPLConfig()
    if mode == "points":
        cfg.batch_norm_mode = "points"
    torch.manual_seed(0); np.random.seed(0)
    nets[mode] = (KPFCNN(cfg, np.arange(9), []).to(dev).eval(), cfg)
batches = []
for s in range(2):
    pts, feats, labels, lens = synthetic.make_inputs(s, wl["spheres"], wl["points"], wl["radius"], nets["reference"][1].in_features_dim)
    batches.append(pyramid.build_batch(nets["reference"][1], torch.from_numpy(pts).to(dev), torch.from_numpy(feats).to(dev),
                                       torch.from_numpy(labels).to(dev), lens, wl["limits"]))
times = {a: [] for a in arms}
launches, folds = {}, {}
with torch.no_grad():
    for it in range(args.warmup + args.reps):
        for arm in arms:
            net, cfg = nets["reference" if arm == "reference" else "points"]
            ops.BN_FOLD = arm != "fold_off"                      # (read at every call; a build without the fold ignores it)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            before, fbefore = lib.ws_launch_count(), getattr(ops, "bn_fold_launches", 0)
            e0.record(); net(batches[it % 2], cfg); e1.record()
            torch.cuda.synchronize()
            launches[arm] = int(lib.ws_launch_count() - before)
            folds[arm] = int(getattr(ops, "bn_fold_launches", 0) - fbefore)
            if it >= args.warmup:
                times[arm].append(e0.elapsed_time(e1))
res = {a: dict(ms_mean=float(np.mean(t)), ms_median=float(np.median(t)), ms_min=float(min(t)), ms_max=float(max(t)),
               library_launches_per_forward=launches[a], of_which_fold=folds[a]) for a, t in times.items()}
res["rows_level0"] = int(batches[0].points[0].shape[0])
res["tag"] = args.tag
os.makedirs(os.path.join(REPO, "bench_outputs"), exist_ok=True)
json.dump(res, open(os.path.join(REPO, "bench_outputs", "bn_fold_ab%s.json" % (("_" + args.tag) if args.tag else "")), "w"), indent=1)
print(json.dumps(res))
