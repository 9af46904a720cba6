"""active.select_points on the device against the numpy recipe of tests/active_ref.py on the host: one cloud of Vaihingen-
like and of DALES-like size, k = 5000, with no used ids and with 20 * k of them.

The device time is the wall time of select_points plus the host read of the k ids (votes already resident).  The host is
timed twice: the restatement with a mask in place of the removal loop (`numpy_mask_ms`), and the reference's own removal
loop, one np.delete(np.where()) per used id, on a sample of the used ids and scaled to all of them
(`numpy_loop_ms_extrapolated`: the loop is linear in the number of used ids and would run for minutes)."""
import json, os, sys, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
import active_ref
from weasal_amd import _lib, active

K = 5000
LOOP_SAMPLE = 40
dev = torch.device("cuda:0")
class_w = np.ones(9)
lib = _lib.lib()


class Votes:
    def __init__(self, probs):
        self.probs = [probs]


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


rows = []
for name, n in (("vaihingen", 300_000), ("dales", 2_000_000)):
    probs = active_ref.synthetic_votes(1, n, 9)
    votes = Votes(torch.from_numpy(probs).to(dev))
    for n_used in (0, 20 * K):
        used = np.random.default_rng(2).choice(n, size=n_used, replace=False).astype(np.int64)
        wall(lambda: active.select_points(votes, 0, class_w, used, K).cpu(), 3)                 # warm-up
        before = lib.ws_launch_count()
        got = active.select_points(votes, 0, class_w, used, K).cpu().numpy()
        launches = lib.ws_launch_count() - before
        gpu = wall(lambda: active.select_points(votes, 0, class_w, used, K).cpu(), 20)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); ids = active.select_points(votes, 0, class_w, used, K); e1.record(); torch.cuda.synchronize()
        cpu = []
        for _ in range(3):
            t0 = time.perf_counter(); want = active_ref.select_points(probs, class_w, used, K); cpu.append((time.perf_counter() - t0) * 1e3)
        loop_ms = 0.0
        if n_used:
            order = active_ref.order(active_ref.point_scores(probs, class_w)[2])
            t0 = time.perf_counter(); active_ref.remove_used_reference(order, used[:LOOP_SAMPLE])
            loop_ms = (time.perf_counter() - t0) * 1e3 / LOOP_SAMPLE * n_used
        rows.append(dict(workload=name, n=n, k=K, used=n_used, gpu_ms_median=float(np.median(gpu)), gpu_ms_min=float(min(gpu)),
                         gpu_stream_ms=float(e0.elapsed_time(e1)), launches=int(launches), numpy_mask_ms=float(np.median(cpu)),
                         numpy_loop_ms_extrapolated=float(loop_ms), ids_differ=int(len(np.setdiff1d(got, want)))))
        print(json.dumps(rows[-1]), flush=True)
res = dict(rows=rows, cpu_threads=os.environ.get("OMP_NUM_THREADS"),
           cpu_model=[l.split(":")[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0])
os.makedirs(os.path.join(REPO, "bench_outputs"), exist_ok=True)
json.dump(res, open(os.path.join(REPO, "bench_outputs", "active_bench.json"), "w"))
print(json.dumps(res))
