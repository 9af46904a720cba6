"""KPFCNN_mprm.region_mprm_loss forward + backward on the list path (a dense A [R, N] built on the host and uploaded every
step) against the device path (regions.SphereRegions through ops.region_mean), on the SAME regions, at the shapes of BASELINE
config 1: in_radius 18, sub_radius 5, dl 0.24, 'reduced' anchors plus overlap anchors, batch_num 3 spheres, K = 4 maps of
C = 9 classes.  One synthetic tile: a rough ground sheet of 120 m x 120 m at 0.24 m spacing with 15 % of the points up to
12 m above it, nine classes in patches.  Separately: regions.cut_regions per batch.

Timing: both paths alternate in one loop after warm-up; per call the HIP-event time between a record before the call and one
after its backward (a start event on an idle stream completes at once, so the host work of the list path -- building and
uploading A -- is inside it) and the wall time of the call ending in a synchronise.  The cut is wall time including its one
host read.  Medians; no pass/fail threshold is attached.  The two paths' losses and gradients are compared in the output."""
import json, os, sys, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from weasal_amd import _lib, anchors, regions
from weasal_amd.architectures import KPFCNN_mprm

IN_RADIUS, SUB_RADIUS, DL, C, K, B, SIDE = 18.0, 5.0, 0.24, 9, 4, 3, 120.0
WARMUP, REPS = 3, 15
dev = torch.device("cuda:0")
lib = _lib.lib()
rng = np.random.RandomState(0)
g = np.arange(0.0, SIDE, DL)
xy = np.stack(np.meshgrid(g, g, indexing='ij'), axis=-1).reshape(-1, 2) + rng.uniform(-0.05, 0.05, size=(len(g) ** 2, 2))
z = 3.0 * np.sin(xy[:, 0] / 40.0) + 2.0 * np.cos(xy[:, 1] / 55.0) + rng.normal(0, 0.03, len(xy))
z += np.where(rng.uniform(size=len(xy)) < 0.15, rng.uniform(0, 12, len(xy)), 0.0)
points = np.concatenate([xy, z[:, None]], axis=1).astype(np.float32)
labels = ((np.floor(xy[:, 0] / 9.0) + np.floor(xy[:, 1] / 13.0)) % C).astype(np.int32)
P, L = torch.from_numpy(points).to(dev), torch.from_numpy(labels).to(dev)
base = anchors.anchors_with_points(P, L, anchors.get_anchors(P, SUB_RADIUS, 'reduced'), SUB_RADIUS, C)
aset = anchors.update_anchors(base, P, SUB_RADIUS)
regions.prepare(aset)
centres = np.array([[40.0, 40.0, 2.0], [75.0, 60.0, 1.0], [55.0, 85.0, 3.0]], np.float64)[:B]
inds = []
for c in centres:                                                              # the sampler's members: ascending ids inside in_radius
    d = P.double() - torch.from_numpy(c).to(dev)
    inds.append(torch.nonzero((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= IN_RADIUS * IN_RADIUS).reshape(-1))
lengths = np.array([int(i.shape[0]) for i in inds], np.int64)
input_inds = torch.cat(inds)
batch_labels = L[input_inds].long()
n = int(lengths.sum())


def cut():
    return regions.cut_regions([aset], np.zeros(B, np.int64), centres, input_inds, lengths, batch_labels, IN_RADIUS, SUB_RADIUS, C)


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn(); torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


wall(cut, WARMUP)
before = lib.ws_launch_count()
sr = cut()
cut_launches = lib.ws_launch_count() - before
t_cut = wall(cut, REPS)
region, region_lb = sr.to_lists()


class Net:
    criterion_multi = torch.nn.BCEWithLogitsLoss()


cams = [torch.from_numpy(rng.standard_normal((n, C)).astype(np.float32)).to(dev) for _ in range(K)]
paths = {"list": (region, region_lb, lengths), "device": (sr, None, None)}


def step(name):
    leaves = [m.clone().requires_grad_(True) for m in cams]
    loss = KPFCNN_mprm.region_mprm_loss(Net(), leaves, *paths[name])
    loss.backward()
    return loss.detach(), [m.grad for m in leaves]


times = {name: {"event": [], "wall": []} for name in paths}
for it in range(WARMUP + REPS):
    for name in paths:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        e0.record(); step(name); e1.record()
        torch.cuda.synchronize()
        if it >= WARMUP:
            times[name]["wall"].append((time.perf_counter() - t0) * 1e3)
            times[name]["event"].append(e0.elapsed_time(e1))
(l_list, g_list), (l_dev, g_dev) = step("list"), step("device")
grad_rel = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(g_dev, g_list))
res = dict(in_radius=IN_RADIUS, sub_radius=SUB_RADIUS, dl=DL, tile_points=int(points.shape[0]), anchors=len(aset),
           overlap_anchors=len(aset) - aset.n_base, spheres=B, rows=n, lengths=lengths.tolist(), regions=len(sr), nnz=sr.nnz,
           dense_a_megabytes=len(sr) * n * 4 / 1e6, maps=K, classes=C,
           list_event_ms_median=float(np.median(times["list"]["event"])), list_wall_ms_median=float(np.median(times["list"]["wall"])),
           list_wall_ms_min=float(min(times["list"]["wall"])),
           device_event_ms_median=float(np.median(times["device"]["event"])), device_wall_ms_median=float(np.median(times["device"]["wall"])),
           device_wall_ms_min=float(min(times["device"]["wall"])),
           cut_wall_ms_median=float(np.median(t_cut)), cut_wall_ms_min=float(min(t_cut)), cut_launches=int(cut_launches),
           loss_list=float(l_list), loss_device=float(l_dev), grad_rel_device_vs_list=grad_rel, warmup=WARMUP, reps=REPS,
           cpu_threads=os.environ.get("OMP_NUM_THREADS"),
           cpu_model=[l.split(":")[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0])
os.makedirs(os.path.join(REPO, "bench_outputs"), exist_ok=True)
json.dump(res, open(os.path.join(REPO, "bench_outputs", "region_loss_ab.json"), "w"))
print(json.dumps(res))
