"""One calibration batch, two ways in one process: the older route (an un-limited pyramid.build_batch counted by
calibration.NeighborhoodCalibrator; without transposed tables, which a calibration never reads) and
calibration.DeviceCalibrator.update (count-only pyramid, no index matrix).  Shapes: the benchmark's DALES batch (8 spheres of
50 000 synthetic points) under the rigid DALES configuration and under `dales_deform`, whose un-limited rows are the widest.

Timing: after warm-up the two routes alternate, REPS calls each, wall time of a call ending in a synchronise; both draw
their grid orientations from a RandomState in the same state.  Medians, minima, maxima, the ratio of the medians, and the
peak device memory one call of each route adds (torch's allocator; the search workspaces of the library are not in it,
they are the same for both).  The condition reported per shape: the new route's median lies below the older route's by
more than the older route's own min-max spread.  No pass/fail exit status.
With `--calibrate`: one full calibration.calibrate on the two clouds of tests/golden/g15_sampler.npz, timed once."""
import json, os, sys, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from weasal_amd import calibration, config as wcfg, pyramid, synthetic

WARMUP, REPS = 3, 15
dev = torch.device("cuda:0")


def one_shape(workload):
    wl = synthetic.WORKLOADS[workload]
    cfg = getattr(wcfg, wl["config"])()
    p, f, l, le = synthetic.make_inputs(0, wl["spheres"], wl["points"], wl["radius"], cfg.in_features_dim)
    p, f, l = (torch.from_numpy(a).to(dev) for a in (p, f, l))
    hist_n = calibration.histogram_size(cfg)
    older = calibration.NeighborhoodCalibrator(cfg)
    new = calibration.DeviceCalibrator(cfg, dev)

    def run_older():
        older.update(pyramid.build_batch(cfg, p, f, l, le, (), with_tables=False, rng=np.random.RandomState(5)))

    def run_new():
        new.update(p, le, rng=np.random.RandomState(5))
    routes = {"older": run_older, "new": run_new}
    times = {k: [] for k in routes}
    for it in range(WARMUP + REPS):
        for name, fn in routes.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= WARMUP:
                times[name].append((time.perf_counter() - t0) * 1e3)
    same = bool(torch.equal(older.hists, new.hists))
    peak = {}
    for name, fn in routes.items():
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.max_memory_allocated(dev)
        fn()
        torch.cuda.synchronize()
        peak[name] = int(torch.cuda.max_memory_allocated(dev) - before)
    stat = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), spread=float(max(v) - min(v)))
    st = {k: stat(v) for k, v in times.items()}
    widest = [int(np.nonzero(row)[0].max()) if row.any() else 0 for row in new.hists.cpu().numpy()]
    return dict(workload=workload, points=int(p.shape[0]), spheres=int(len(le)), hist_n=hist_n, widest_row_per_layer=widest,
                histograms_identical=same, wall_ms=st, ratio_older_over_new=st["older"]["median"] / st["new"]["median"],
                condition_met=bool(st["older"]["median"] - st["new"]["median"] > st["older"]["spread"]),
                peak_bytes_one_call=peak, warmup=WARMUP, reps=REPS)


def full_calibration():
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from test_sampler_cpu import golden_scene
    from weasal_amd.sampler import SphereSampler
    g = np.load(os.path.join(REPO, "tests", "golden", "g15_sampler.npz"))
    clouds, _, _ = golden_scene(g)
    cfg = wcfg.DALESPLConfig()
    cfg.in_radius, cfg.first_subsampling_dl, cfg.batch_num, cfg.augment_noise = float(g['in_radius']), float(g['dl']), 4, 0.0
    sampler = SphereSampler(cfg, [(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)) for a, b in clouds],
                            label_values=g['label_values'], seed=3)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    try:
        res = calibration.calibrate(sampler, cfg)
        out = dict(converged=True, steps=res.steps, batch_limit=res.batch_limit, neighborhood_limits=[int(v) for v in res.neighborhood_limits])
    except calibration.CalibrationError as e:
        out = dict(converged=False, steps=len(e.b), last_batch_limit=e.batch_limit[-1], last_estim_b=e.estim_b[-1])
    torch.cuda.synchronize()
    out.update(seconds=time.perf_counter() - t0, clouds=[int(len(a)) for a, _ in clouds], in_radius=cfg.in_radius, batch_num=cfg.batch_num)
    return out


if __name__ == "__main__":
    for workload in ("dales", "dales_deform"):
        r = one_shape(workload)
        print(json.dumps(r))
        w = r["wall_ms"]
        print("# %-12s older %.2f ms (min %.2f, max %.2f)  new %.2f ms (min %.2f, max %.2f)  ratio %.2f  condition %s  peak %s"
              % (workload, w["older"]["median"], w["older"]["min"], w["older"]["max"], w["new"]["median"], w["new"]["min"],
                 w["new"]["max"], r["ratio_older_over_new"], r["condition_met"], r["peak_bytes_one_call"]))
    if "--calibrate" in sys.argv:
        print(json.dumps(dict(full_calibration_g15=full_calibration())))
