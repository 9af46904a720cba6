"""The three per-sphere attention forms of KPFCNN_mprm (spatial_att, channel_att, ele_att), forward + backward, on the loop
the modules take with WEASAL_ATT_KERNELS=0 (torch.matmul / softmax per sphere) against ops.sphere_attention /
ops.channel_attention (weasal_amd/csrc/attention.hip), on the SAME operands, at config 1's widths (out_dim 256: dq 32, dv 256,
channel c 32, elevation c 256) and two sets of sphere sizes: the level-2 sizes of the synthetic config-1 batch
(2 spheres of 3 000 points, R = 4 m, dl0 0.24) and 3 x 2 000 rows (the real sampler's level-2 sizes at in_radius 18).

Timing: both paths alternate in one loop after warm-up; per call the HIP-event time between a record before the call and one
after its backward, and the wall time of the call ending in a synchronise.  Medians and the min-max spread of REPS calls; the
library's launch count per call (ws_launch_count; the loop's torch kernels are not counted by it: its count is the number of
torch ops it issues, reported as 0 here) and the peak memory of one call.  No pass/fail threshold is attached."""
import json, os, sys, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from weasal_amd import _lib, config as wcfg, ops, pyramid, synthetic

WARMUP, REPS = 5, 15
dev = torch.device("cuda:0")
lib = _lib.lib()


def spans(lengths):
    out, s = [], 0
    for n in lengths:
        out.append((s, s + int(n)))
        s += int(n)
    return out


def loop_spatial(q, k, v, lengths):
    outs, outs_n = [], []
    for a, b in spans(lengths):
        att = torch.matmul(torch.softmax(torch.matmul(q[a:b], k[a:b].T), dim=-1), v[a:b])
        outs.append(att)
        outs_n.append(att / float(b - a))
    return torch.cat(outs, 0), torch.cat(outs_n, 0)


def loop_channel(x1, x2, val, lengths, max_minus):
    outs = []
    for a, b in spans(lengths):
        e = torch.matmul(x1[a:b].T, x2[a:b])
        if max_minus:
            e = torch.max(e, -1, keepdim=True)[0].expand_as(e) - e
        outs.append(torch.matmul(val[a:b], torch.softmax(e, dim=-1)))
    return torch.cat(outs, 0)


def config1_level2_lengths():
    wl = synthetic.WORKLOADS["vaihingen_wl"]
    cfg = wcfg.Vaihingen3DWLConfig()
    pts, feats, labels, lens = synthetic.make_inputs(5150, wl["spheres"], wl["points"], wl["radius"], cfg.in_features_dim)
    np.random.seed(31)
    batch = pyramid.build_batch(cfg, torch.from_numpy(pts).to(dev), torch.from_numpy(feats).to(dev),
                                torch.from_numpy(labels).to(dev), lens, wl["limits"])
    return [int(v) for v in batch.lengths_host[2]]


def forms(lengths, g):
    n = sum(lengths)
    r = lambda w, amp=1.0: ((torch.rand((n, w), generator=g) * 2 - 1) * amp).to(dev)
    q, k, v, gs = r(32, 0.5), r(32, 0.5), r(256), (r(256), r(256))
    c1, c2, cv, gc = r(32, 0.5), r(32, 0.5), r(32), r(32)
    e1, e2, ev, ge = r(256, 0.2), r(256, 0.2), r(256), r(256)

    def spatial(fn):
        a, b, c = (t.clone().requires_grad_(True) for t in (q, k, v))
        att, xn = fn(a, b, c, lengths)
        ((att * gs[0]).sum() + (xn * gs[1]).sum()).backward()
        return [att.detach(), xn.detach(), a.grad, b.grad, c.grad]

    def channel(fn, ops_, gout, mm):
        a, b, c = (t.clone().requires_grad_(True) for t in ops_)
        out = fn(a, b, c, lengths, mm)
        (out * gout).sum().backward()
        return [out.detach(), a.grad, b.grad, c.grad]
    return {
        "spatial dq=32 dv=256": {"loop": lambda: spatial(loop_spatial), "kernels": lambda: spatial(ops.sphere_attention)},
        "channel c=32 (max-minus)": {"loop": lambda: channel(loop_channel, (c1, c2, cv), gc, True),
                                     "kernels": lambda: channel(ops.channel_attention, (c1, c2, cv), gc, True)},
        "elevation c=256": {"loop": lambda: channel(loop_channel, (e1, e2, ev), ge, False),
                            "kernels": lambda: channel(ops.channel_attention, (e1, e2, ev), ge, False)},
    }


def measure(paths):
    times = {name: {"event": [], "wall": []} for name in paths}
    for it in range(WARMUP + REPS):
        for name, fn in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            if it >= WARMUP:
                times[name]["wall"].append((time.perf_counter() - t0) * 1e3)
                times[name]["event"].append(e0.elapsed_time(e1))
    out = {}
    for name, fn in paths.items():
        before = lib.ws_launch_count()
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(); base = torch.cuda.memory_allocated()
        fn(); torch.cuda.synchronize()
        t = times[name]
        out[name] = dict(event_ms_median=float(np.median(t["event"])), event_ms_min=float(min(t["event"])), event_ms_max=float(max(t["event"])),
                         wall_ms_median=float(np.median(t["wall"])), wall_ms_min=float(min(t["wall"])), wall_ms_max=float(max(t["wall"])),
                         library_launches=int(lib.ws_launch_count() - before),
                         peak_extra_megabytes=(torch.cuda.max_memory_allocated() - base) / 1e6)
    a, b = paths["kernels"](), paths["loop"]()
    out["max_rel_difference"] = max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for x, y in zip(a, b))
    return out


res = dict(warmup=WARMUP, reps=REPS, cpu_threads=os.environ.get("OMP_NUM_THREADS"), shapes={})
g = torch.Generator().manual_seed(0)
for tag, lengths in (("config 1 level 2", config1_level2_lengths()), ("3 x 2000", [2000, 2000, 2000])):
    res["shapes"][tag] = dict(lengths=lengths, forms={name: measure(paths) for name, paths in forms(lengths, g).items()})
os.makedirs(os.path.join(REPO, "bench_outputs"), exist_ok=True)
json.dump(res, open(os.path.join(REPO, "bench_outputs", "attention_ab.json"), "w"), indent=1)
print(json.dumps(res))
