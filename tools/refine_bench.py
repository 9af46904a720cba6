"""refine.refine_cloud on the device against the numpy restatement of tests/refine_ref.py on the host: one synthetic tile of
DALES-like size (N = 2 000 000 points, C = 9 classes, 4 000 anchors of 50..4000 points), threshold 10 %.

The device time is the wall time of refine_cloud (votes and anchors already resident) plus the one host read of a
refinement, counts and status words; `gpu_stream_ms` is the HIP-event time of the same call.  The host time is what a
user without this operator pays after a voting pass: the device-to-host copy of the [N, C] votes (`d2h_ms`), then the
restatement (per-point weak labels, emptying, counts).  No pass/fail threshold is attached."""
import json, os, sys, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
import active_ref, refine_ref
from weasal_amd import _lib, refine, tester

N, C, ANCHORS, THRESHOLD = 2_000_000, 9, 4000, 10
dev = torch.device("cuda:0")
lib = _lib.lib()
label_values = np.arange(1, C + 1)


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


probs = active_ref.synthetic_votes(1, N, C)
ptr, idx, labels = active_ref.synthetic_anchors(2, N, ANCHORS, C)
votes = tester.VoteAccumulator([N], C, dev)
votes.probs[0].copy_(torch.from_numpy(probs).to(dev))
ptr_d, idx_d = torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)
out = torch.empty(N, dtype=torch.int32, device=dev)


def device_run():
    counts = torch.zeros(C + 2, dtype=torch.int64, device=dev)
    status = refine.new_status(dev)
    refine.refine_cloud(votes, 0, ptr_d, idx_d, labels, THRESHOLD, label_values=label_values, counts=counts, out=out, status=status)
    return refine.read_counts(counts, status)


wall(device_run, 3)                                                            # warm-up
before = lib.ws_launch_count()
got_counts = device_run()
launches = lib.ws_launch_count() - before
gpu = wall(device_run, 20)
counts = torch.zeros(C + 2, dtype=torch.int64, device=dev)
status = refine.new_status(dev)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
refine.refine_cloud(votes, 0, ptr_d, idx_d, labels, THRESHOLD, label_values=label_values, counts=counts, out=out, status=status)
e1.record(); torch.cuda.synchronize()

d2h, cpu = [], []
for _ in range(3):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    host_probs = votes.probs[0].cpu().numpy()
    t1 = time.perf_counter()
    want_labels, want_counts = refine_ref.refine_cloud(host_probs, label_values, N, ptr, idx, labels, THRESHOLD, n_counts=C + 2)
    t2 = time.perf_counter()
    d2h.append((t1 - t0) * 1e3); cpu.append((t2 - t1) * 1e3)
res = dict(n=N, c=C, anchors=ANCHORS, nnz=int(ptr[-1]), threshold=THRESHOLD, gpu_ms_median=float(np.median(gpu)),
           gpu_ms_min=float(min(gpu)), gpu_stream_ms=float(e0.elapsed_time(e1)), launches=int(launches),
           d2h_ms=float(np.median(d2h)), numpy_ms=float(np.median(cpu)), host_total_ms=float(np.median(d2h) + np.median(cpu)),
           labels_differ=int((out.cpu().numpy() != want_labels).sum()), counts_equal=bool(np.array_equal(got_counts, want_counts)),
           emptied=int(want_counts[10]), cpu_threads=os.environ.get("OMP_NUM_THREADS"),
           cpu_model=[l.split(":")[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0])
os.makedirs(os.path.join(REPO, "bench_outputs"), exist_ok=True)
json.dump(res, open(os.path.join(REPO, "bench_outputs", "refine_bench.json"), "w"))
print(json.dumps(res))
