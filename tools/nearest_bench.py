"""The exact nearest-neighbour search (ops.nearest_neighbors behind tester.nearest_projection(P, S)) against the route the
callers used before it, tester.nearest_projection(P, S, radius) -- the K1 radius search with one column, in chunks of 4 M
queries, with a host read per pass -- on one GPU, in one process.

(a) the re-projection of a DALES tile: every point of a 12 M point tile (500 x 500 m of rolling ground with scattered
    vegetation, listed in 2 m squares like a tile that was written strip by strip) against its grid sub-cloud of about 3 M
    barycentres (datasets/DALES_PseudoLabel.py:888-893);
(b) the reverse direction of refine.roundtrip_projection: every sub-cloud point against the full tile.

The two routes' outputs are compared before timing: rows may differ only where the float32 route cannot tell two
candidates apart (their float64 distances agree to 1e-6 relative).  After 3 warm-ups the routes alternate, 20 repetitions:
wall time around a call that ends in a synchronise for both, HIP events as well for the new one.  Derived: the bytes the
algorithm needs from the shapes -- (nq + ns) * 12 + nq * 4 plus the grid tables (one float4 per support in cell order,
4 bytes per cell start, 4 per support for the order) -- and their share of the 8 TB/s HBM peak at the median event time;
host reads per call (new: 0; old: two per radius search, its maximum count and the size of the boolean selection).
Medians, minima and maxima; no pass/fail threshold.  `--part a` / `--part b` runs one part."""
import json, os, sys, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from weasal_amd import ops, tester

WARMUP, REPS, HBM_PEAK = 3, 20, 8.0e12
dev = torch.device("cuda:0")
stat = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
part = sys.argv[sys.argv.index("--part") + 1] if "--part" in sys.argv else "ab"
N_FULL = int(sys.argv[sys.argv.index("--points") + 1]) if "--points" in sys.argv else 12_000_000
DL = 0.29
res = dict(warmup=WARMUP, reps=REPS, full_points=N_FULL, dl=DL)

g = torch.Generator(device=dev).manual_seed(0)
xy = torch.rand((N_FULL, 2), device=dev, generator=g) * 500.0
ground = 8.0 * torch.sin(xy[:, 0] / 60.0) * torch.cos(xy[:, 1] / 45.0)
veg = (torch.rand(N_FULL, device=dev, generator=g) < 0.25) * torch.rand(N_FULL, device=dev, generator=g) * 12.0
z = ground + veg + 0.03 * torch.randn(N_FULL, device=dev, generator=g)
order = torch.argsort((xy[:, 1] / 2.0).floor() * 250 + (xy[:, 0] / 2.0).floor(), stable=True)
full = torch.stack([xy[:, 0], xy[:, 1], z], 1)[order].contiguous()
del xy, ground, veg, z, order
while True:          # the cell that leaves about a quarter of the points
    sub = ops.grid_subsample(full, np.array([N_FULL], np.int32), DL)[0].contiguous()
    if sub.shape[0] <= 0.27 * N_FULL:
        break
    DL = round(DL * 1.1, 3)
res.update(dl=DL, sub_points=int(sub.shape[0]))
radius = DL * 3 ** 0.5

searches = [0]
_radius_neighbors = ops.radius_neighbors


def counted(*a, **k):
    searches[0] += 1
    return _radius_neighbors(*a, **k)


ops.radius_neighbors = counted


def compare(Q, S):
    new, old = tester.nearest_projection(Q, S), tester.nearest_projection(Q, S, radius)
    rows = torch.nonzero(new != old).reshape(-1)
    q64 = Q[rows].double()
    dn = (q64 - S[new[rows].long()].double()).square().sum(1)
    do = (q64 - S[old[rows].long()].double()).square().sum(1)
    rel = ((dn - do).abs() / do.clamp_min(1e-300)).max().item() if rows.numel() else 0.0
    return dict(rows_that_differ=int(rows.numel()), new_is_never_farther=bool((dn <= do).all().item()),
                max_relative_d2_difference=rel, equal_outside_float32_near_ties=bool(rel <= 1e-6))


def measure(Q, S):
    nq, ns = Q.shape[0], S.shape[0]
    out = dict(queries=nq, supports=ns, outputs=compare(Q, S))
    searches[0] = 0
    tester.nearest_projection(Q, S, radius)
    out["host_reads_per_call"] = dict(new=0, old=2 * searches[0])
    wall, event = {"exact": [], "radius_route": []}, []
    for it in range(WARMUP + REPS):
        for name in ("exact", "radius_route"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            e0.record()
            r = tester.nearest_projection(Q, S) if name == "exact" else tester.nearest_projection(Q, S, radius)
            e1.record()
            torch.cuda.synchronize()
            t = (time.perf_counter() - t0) * 1e3
            del r
            if it >= WARMUP:
                wall[name].append(t)
                if name == "exact":
                    event.append(e0.elapsed_time(e1))
    cells = 4 * ns + 64
    needed = (nq + ns) * 12 + nq * 4 + ns * 16 + cells * 4 + ns * 4
    med = float(np.median(event))
    out.update(wall_ms={k: stat(v) for k, v in wall.items()}, exact_event_ms=stat(event), bytes_needed=needed,
               achieved_GBps=needed / (med * 1e-3) / 1e9, share_of_hbm_peak=needed / (med * 1e-3) / HBM_PEAK,
               speedup_median_wall=float(np.median(wall["radius_route"]) / np.median(wall["exact"])))
    return out


if "a" in part:
    res["reprojection"] = measure(full, sub)
if "b" in part:
    res["reverse"] = measure(sub, full)
print(json.dumps(res))
