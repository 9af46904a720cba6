"""anchors.anchors_with_points + update_anchors on the device against the sklearn / numpy host path the reference takes
(datasets/DALES_WeakLabel.py:201-269): one synthetic tile of DALES-like size, N = 2 000 000 points over 500 m x 500 m (a
rough ground sheet, 15 % of the points up to 25 m above it), nine classes in patches, sub_radius = 5, 'reduced' lattice.

The device time is the wall time of the two calls with the points and labels resident, every host read they make
included (medians after warm-up); `gpu_members_ms` / `gpu_update_ms` split it.  The host time is what a user without these
operators pays: the device-to-host copy of the points (`d2h_ms`), the KD-tree (`tree_ms`), one query_radius and one
np.unique per anchor (`members_ms`), one tree query over the anchors and one intersection per neighbouring pair
(`update_ms`); it runs once.  The two results are compared (lists and label rows exactly, as multisets for the overlap
anchors).  No pass/fail threshold is attached."""
import json, os, sys, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
from weasal_amd import _lib, anchors

N, C, SUB_RADIUS, METHOD = 2_000_000, 9, 5.0, 'reduced'
dev = torch.device("cuda:0")
lib = _lib.lib()
rng = np.random.RandomState(0)
xy = rng.uniform(0, 500, size=(N, 2))
z = 3.0 * np.sin(xy[:, 0] / 40.0) + 2.0 * np.cos(xy[:, 1] / 55.0) + rng.normal(0, 0.05, N)
z += np.where(rng.uniform(size=N) < 0.15, rng.uniform(0, 25, N), 0.0)
points = np.concatenate([xy, z[:, None]], axis=1).astype(np.float32)
labels = ((np.floor(xy[:, 0] / 37.0) + np.floor(xy[:, 1] / 53.0)) % C).astype(np.int32)
P, L = torch.from_numpy(points).to(dev), torch.from_numpy(labels).to(dev)


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn(); torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


grid = anchors.get_anchors(P, SUB_RADIUS, METHOD)
state = {}


def members():
    state["base"] = anchors.anchors_with_points(P, L, grid, SUB_RADIUS, C)


def update():
    state["full"] = anchors.update_anchors(state["base"], P, SUB_RADIUS)


def both():
    members(); update()


wall(both, 2)                                                                  # warm-up
before = lib.ws_launch_count()
both()
launches = lib.ws_launch_count() - before
t_both, t_members = wall(both, 7), wall(members, 7)
t_update = wall(update, 7)
base, full = state["base"], state["full"]
res = dict(n=N, c=C, sub_radius=SUB_RADIUS, method=METHOD, anchors_in=int(grid.shape[0]), anchors_kept=len(base),
           nnz=int(base.idx.shape[0]), overlap_anchors=len(full) - full.n_base, overlap_nnz=int(full.idx.shape[0] - base.idx.shape[0]),
           gpu_ms_median=float(np.median(t_both)), gpu_ms_min=float(min(t_both)), gpu_members_ms=float(np.median(t_members)),
           gpu_update_ms=float(np.median(t_update)), launches=int(launches), cpu_threads=os.environ.get("OMP_NUM_THREADS"),
           cpu_model=[l.split(":")[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0])
try:
    from sklearn.neighbors import KDTree
except ImportError:
    KDTree = None
if KDTree is not None and "--no-host" not in sys.argv:
    torch.cuda.synchronize(); t0 = time.perf_counter()
    host_points = P.cpu().numpy()
    t1 = time.perf_counter()
    tree = KDTree(host_points, leaf_size=10)
    t2 = time.perf_counter()
    kept, lists, rows = [], [], []
    for a in range(grid.shape[0]):
        inds = tree.query_radius(grid[a].reshape(1, -1), r=SUB_RADIUS)[0]
        if inds.shape[0] > 0:
            row = np.zeros(C, np.int64)
            row[np.unique(labels[inds])] = 1
            kept.append(a); lists.append(np.sort(inds)); rows.append(row)
    t3 = time.perf_counter()
    centres = grid[kept]
    near = KDTree(centres, leaf_size=10).query_radius(centres, r=1.5 * SUB_RADIUS)
    data = np.asarray(tree.data)
    new = []
    for i in range(len(lists)):
        for j in near[i][near[i] > i]:
            if (rows[i] != rows[j]).any():
                common = np.intersect1d(lists[i], lists[j], assume_unique=True)
                if common.shape[0]:
                    new.append((tuple(common.tolist()), tuple((rows[i] * rows[j]).tolist()), data[common].mean(axis=0)))
    t4 = time.perf_counter()
    ptr, idx = full.ptr.cpu().numpy(), full.idx.cpu().numpy()
    same_base = bool(np.array_equal(base.kept, kept) and np.array_equal(base.lb, np.asarray(rows)) and
                     np.array_equal(idx[:ptr[full.n_base]], np.concatenate(lists)))
    got_new = sorted((tuple(idx[ptr[a]:ptr[a + 1]].tolist()), tuple(full.lb[a].tolist())) for a in range(full.n_base, len(full)))
    res.update(d2h_ms=(t1 - t0) * 1e3, tree_ms=(t2 - t1) * 1e3, members_ms=(t3 - t2) * 1e3, update_ms=(t4 - t3) * 1e3,
               host_total_ms=(t4 - t0) * 1e3, base_equal=same_base, overlap_equal=bool(got_new == sorted(n[:2] for n in new)))
os.makedirs(os.path.join(REPO, "bench_outputs"), exist_ok=True)
json.dump(res, open(os.path.join(REPO, "bench_outputs", "anchors_bench.json"), "w"))
print(json.dumps(res))
