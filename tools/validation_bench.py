"""The votes of one DALES-shaped validation batch, three ways in one process: tester.VoteAccumulator.update_batch (one
launch, ws_validation_update) with the all-pairs mask and with the centre mask, and the per-sphere loop of
VoteAccumulator.update (one ws_vote_update launch per sphere).  Shape of BASELINE config 3: 8 spheres of about 50 000 rows,
9 classes, two clouds of 2 M rows; every cloud is a square tile of uniformly scattered points, its four spheres are discs
whose centres lie 1.1 radii apart on a line, so that only neighbours overlap; rows ascend inside a sphere.

Timing: after warm-up the three forms alternate; per call the HIP-event time between a record before and one after the call,
and the wall time of the call ending in a synchronise.  The loop gets its lengths and cloud ids from the host here; the
blocking `.tolist()` read it makes when they arrive as device tensors is timed separately, on an idle stream (in a
validation loop it would wait for the forward pass as well).  Medians, minima and maxima; no pass/fail threshold.
With `--confusion` the batched call also counts the epoch confusion (validation.Validator.update)."""
import json, os, sys, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from weasal_amd import _lib, tester, validation

N_CLOUD, SPHERES_PER_CLOUD, ROWS, C = 2_000_000, 4, 50_000, 9
WARMUP, REPS = 5, 50
dev = torch.device("cuda:0")
lib = _lib.lib()
rng = np.random.default_rng(0)
radius = float(np.sqrt(ROWS / N_CLOUD / np.pi))                                  # unit square: a disc holding ROWS points
tiles, centres, inds = [], [], []
for t in range(2):
    xy = torch.from_numpy(rng.random((N_CLOUD, 2))).to(dev)
    for s in range(SPHERES_PER_CLOUD):
        c = np.array([0.3 + 1.1 * s * radius, 0.4 + 0.1 * t, 0.0])
        d = xy - torch.from_numpy(c[:2]).to(dev)
        inds.append(torch.nonzero(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] < radius * radius).reshape(-1))
        tiles.append(t); centres.append(c)
order = [0, 4, 1, 5, 2, 6, 3, 7]                                                 # the two tiles interleaved, as a sampler draws them
tiles, centres, inds = np.array(tiles)[order], np.array(centres)[order], [inds[o] for o in order]
lengths = np.array([int(i.shape[0]) for i in inds], np.int32)
input_inds = torch.cat(inds)
n = int(lengths.sum())
logits = torch.from_numpy((rng.standard_normal((n, C)) * 2).astype(np.float32)).to(dev)
points0 = torch.zeros((n, 3), device=dev)
labels = torch.from_numpy(rng.integers(0, C, size=n)).to(dev)
lengths_dev, tiles_dev = torch.from_numpy(lengths).to(dev), torch.from_numpy(tiles).to(dev)
masks = validation.overlap_from_centres(tiles, centres, radius)
shared = int(n - torch.cat([torch.unique(torch.cat([i for i, t in zip(inds, tiles) if t == k])) for k in range(2)]).shape[0])

start = [torch.from_numpy(rng.random((N_CLOUD, C), dtype=np.float32)).to(dev) for _ in range(2)]
acc = {}
for name in ("batch_all_pairs", "batch_centres", "loop"):
    acc[name] = tester.VoteAccumulator([N_CLOUD, N_CLOUD], C, dev)
    for p, s in zip(acc[name].probs, start):
        p.copy_(s)
forms = {
    "batch_all_pairs": lambda: acc["batch_all_pairs"].update_batch(logits, lengths, input_inds, tiles),
    "batch_centres": lambda: acc["batch_centres"].update_batch(logits, lengths, input_inds, tiles, overlap=masks),
    "loop": lambda: acc["loop"].update(logits, points0, lengths, input_inds, tiles),
}
if "--confusion" in sys.argv:
    val = validation.Validator([N_CLOUD, N_CLOUD], np.arange(C), [], [labels], dev)
    fields = {"labels": labels, "lengths": lengths, "input_inds": input_inds, "cloud_inds": tiles}
    forms["validator_centres"] = lambda: val.update(logits, fields, overlap=masks)

launches = {}
for name, fn in forms.items():
    before = lib.ws_launch_count()
    fn()
    launches[name] = int(lib.ws_launch_count() - before)
torch.cuda.synchronize()
diff = {name: max(float((a - b).abs().max()) for a, b in zip(acc[name].probs, acc["loop"].probs)) for name in acc}
same_bits = all(torch.equal(a, b) for a, b in zip(acc["batch_all_pairs"].probs, acc["batch_centres"].probs))

times = {name: {"event": [], "wall": []} for name in forms}
tolist = []
for it in range(WARMUP + REPS):
    for name, fn in forms.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        if it >= WARMUP:
            times[name]["wall"].append((time.perf_counter() - t0) * 1e3)
            times[name]["event"].append(e0.elapsed_time(e1))
    torch.cuda.synchronize(); t0 = time.perf_counter()
    lengths_dev.tolist(); tiles_dev.tolist()
    if it >= WARMUP:
        tolist.append((time.perf_counter() - t0) * 1e3)
assert acc["batch_all_pairs"].batch_status.cpu().tolist() == [0, 0, 0]

stat = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
res = dict(clouds=2, cloud_rows=N_CLOUD, spheres=len(lengths), rows=n, lengths=lengths.tolist(), tiles=tiles.tolist(), classes=C,
           rows_listed_more_than_once=shared, overlap_masks=[int(m) for m in masks], launches=launches,
           max_abs_diff_to_loop_after_one_batch=diff, all_pairs_and_centres_bit_identical=bool(same_bits),
           event_ms={k: stat(v["event"]) for k, v in times.items()}, wall_ms={k: stat(v["wall"]) for k, v in times.items()},
           loop_tolist_read_ms_idle_stream=stat(tolist), warmup=WARMUP, reps=REPS, cpu_threads=os.environ.get("OMP_NUM_THREADS"))
print(json.dumps(res))
for name in forms:
    print("# %-18s %d launch(es): events median %.4f ms (min %.4f, max %.4f); wall with synchronise median %.4f ms (min %.4f, max %.4f)"
          % (name, launches[name], *[res["event_ms"][name][k] for k in ("median", "min", "max")],
             *[res["wall_ms"][name][k] for k in ("median", "min", "max")]))
print("# the loop's .tolist() of lengths and cloud ids on an idle stream: median %.4f ms (min %.4f, max %.4f)"
      % tuple(res["loop_tolist_read_ms_idle_stream"][k] for k in ("median", "min", "max")))
