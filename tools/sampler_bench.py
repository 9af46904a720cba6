"""SphereSampler.sample() on a synthetic 2 M-point tile against tests/sampler_ref.py on the host (same draws)."""
import json, os, sys, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
from weasal_amd import config as wcfg
from weasal_amd.sampler import SphereSampler
no_cpu = "--no-cpu" in sys.argv
nb = 10 if no_cpu else 25
dev = torch.device("cuda:0")
cfg = wcfg.DALESPLConfig()
N = 2_000_000
rs = np.random.RandomState(1)
pts = (rs.uniform(0, 1, size=(N, 3)) * np.array([500.0, 500.0, 10.0])).astype(np.float32)
lab = rs.randint(0, 8, size=N).astype(np.int32)
cfg.in_radius = float(np.sqrt(50000 / (N / 250000.0) / np.pi))      # ~50 k points per interior sphere
P, L = torch.from_numpy(pts).to(dev), torch.from_numpy(lab).to(dev)
s = SphereSampler(cfg, [(P, L)], label_values=np.arange(8), seed=2, max_spheres=16, batch_limit=7.5 * 50000)
draws = [s.draw() for _ in range(nb)]
times, sizes = [], []
for d in draws:
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = s.sample(draws=d); torch.cuda.synchronize()
    times.append(time.perf_counter() - t0); sizes.append([int(v) for v in out[3]])
res = dict(in_radius=cfg.in_radius, pot_points=int(s.pot_points[0].shape[0]), gpu_ms=[t * 1e3 for t in times], sizes=sizes)
if not no_cpu:
    import sampler_ref
    t0 = time.perf_counter()
    pot0 = None
    s2 = SphereSampler(cfg, [(P, L)], label_values=np.arange(8), seed=2, max_spheres=16, batch_limit=7.5 * 50000)
    ref = sampler_ref.RefSampler([(pts, lab)], [s2.pot_points[0].cpu().numpy()], [s2.potentials[0].cpu().numpy()], cfg.in_radius)
    res["cpu_tree_build_s"] = time.perf_counter() - t0
    ct = []
    for d in draws[:8]:
        t0 = time.perf_counter(); r = ref.batch(d, 16, 7.5 * 50000, fd=3, lut=np.arange(8)); ct.append(time.perf_counter() - t0)
    res["cpu_ms"] = [t * 1e3 for t in ct]
    res["cpu_threads"] = os.environ.get("OMP_NUM_THREADS"); 
    res["cpu_model"] = [l.split(":")[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0]
    g = np.median(res["gpu_ms"][5:]); b = np.mean([len(x) for x in sizes[5:]])
    res["summary"] = dict(gpu_ms_median=float(g), spheres_per_batch=float(b), gpu_spheres_per_s=float(b / g * 1e3),
                          cpu_ms_median=float(np.median(res["cpu_ms"])))
os.makedirs(os.path.join(REPO, "bench_outputs"), exist_ok=True)
json.dump(res, open(os.path.join(REPO, "bench_outputs", "sampler_bench%s.json" % ("_prof" if no_cpu else "")), "w"))
print(json.dumps(res))
