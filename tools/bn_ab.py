"""Batch normalisation over the points, forward + backward: ops.batch_norm_act (ws_bn_fwd / ws_bn_bwd,
weasal_amd/csrc/batchnorm.hip) against the framework route a 'points' BatchNormBlock takes with WEASAL_BN_KERNELS=0
(nn.BatchNorm1d + add + F.leaky_relu under autograd), on the SAME tensors, at the training shapes of the default benchmark:
the DALES levels (400 000 / 71 000 / 10 339 / 1 547 / 284 rows) at the widths those levels carry with
first_features_dim = 128 (a block's out / 4 and out; the input layer's 64).  Training mode, residual and LeakyReLU present
(the residual block's last call: the widest epilogue).

Timing: the two routes alternate in one loop after warm-up; per call one HIP-event interval around the forward and one
around the backward.  Medians and the min-max spread of REPS calls.  `fwd_fraction_of_peak`: the bytes the forward cannot
avoid -- read y, read residual, write out -- over the event time, as a fraction of the 8 TB/s HBM peak (about 6.3 TB/s is
achievable); `bwd_...`: read dout, out, y, write dy and dresidual.  The tensors of the smaller shapes fit the 256 MiB
Infinity Cache between calls, so their fractions are not HBM rates.  The training forward reads y twice (statistics, then
apply), so the bytes it really moves are 4/3 of the figure's numerator.  No pass/fail threshold is attached."""
import json, os, sys
import numpy as np, torch
import torch.nn.functional as F
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from weasal_amd import _lib, ops

WARMUP, REPS = 5, 15
HBM_PEAK = 8.0e12
SHAPES = [(400000, 32), (400000, 64), (400000, 128), (71000, 64), (71000, 256), (10339, 128), (10339, 512), (1547, 256),
          (1547, 1024), (284, 512), (284, 1024), (284, 2048)]
dev = torch.device("cuda:0")
lib = _lib.lib()


def kernels(y, res, bn):
    return ops.batch_norm_act(y, bn, residual=res, slope=0.1)


def framework(y, res, bn):
    return F.leaky_relu(bn(y) + res, 0.1)


def measure(n, c, g):
    y0, r0, dout = (torch.randn((n, c), generator=g).to(dev) for _ in range(3))
    bns = {name: torch.nn.BatchNorm1d(c, momentum=0.02).to(dev).train() for name in ("kernels", "framework")}
    routes = {"kernels": kernels, "framework": framework}
    times = {name: {"fwd": [], "bwd": []} for name in routes}
    last = {}
    for it in range(WARMUP + REPS):
        for name, fn in routes.items():
            y, r = y0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
            bns[name].zero_grad(set_to_none=True)
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            torch.cuda.synchronize()
            e[0].record(); out = fn(y, r, bns[name]); e[1].record(); out.backward(dout); e[2].record()
            torch.cuda.synchronize()
            if it >= WARMUP:
                times[name]["fwd"].append(e[0].elapsed_time(e[1]))
                times[name]["bwd"].append(e[1].elapsed_time(e[2]))
            last[name] = [out.detach(), y.grad, r.grad, bns[name].weight.grad, bns[name].bias.grad]
    res = {}
    bytes_fwd, bytes_bwd = 3 * n * c * 4, 5 * n * c * 4
    for name in routes:
        f, b = times[name]["fwd"], times[name]["bwd"]
        res[name] = dict(fwd_ms_median=float(np.median(f)), fwd_ms_min=float(min(f)), fwd_ms_max=float(max(f)),
                         bwd_ms_median=float(np.median(b)), bwd_ms_min=float(min(b)), bwd_ms_max=float(max(b)),
                         fwd_fraction_of_peak=bytes_fwd / HBM_PEAK / (float(np.median(f)) * 1e-3),
                         bwd_fraction_of_peak=bytes_bwd / HBM_PEAK / (float(np.median(b)) * 1e-3))
    names = ("out", "dy", "dresidual", "dgamma", "dbeta")
    scale = [b.abs().max().clamp_min(1e-30) for b in last["framework"]]
    res["max_rel_difference"] = {k: float((a - b).abs().max() / s) for k, a, b, s in zip(names, last["kernels"], last["framework"], scale)}
    # the two routes gate by their own outputs: an element whose pre-activation rounds to the other side of zero has its
    # gradient scaled by 1 on one route and by the slope on the other -- counted here, not hidden
    res["elements_beyond_1e-4"] = {k: int(((a - b).abs() > 1e-4 * s).sum()) for k, a, b, s in zip(names, last["kernels"], last["framework"], scale)}
    buf = __import__("ctypes").create_string_buffer(400)
    lib.ws_bn_variant(0, n, c, y0.data_ptr(), c, y0.data_ptr(), c, r0.data_ptr(), c, None, 0, None, 0, 1, 1, buf, 400)
    res["plan"] = buf.value.decode()
    return res


out = dict(warmup=WARMUP, reps=REPS, hbm_peak_bytes_per_s=HBM_PEAK, bn_kernels=ops.BN_KERNELS, shapes={})
g = torch.Generator().manual_seed(0)
for n, c in SHAPES:
    out["shapes"]["%dx%d" % (n, c)] = measure(n, c, g)
    r = out["shapes"]["%dx%d" % (n, c)]
    print("%7d x %4d  kernels fwd %.3f bwd %.3f ms (%.2f / %.2f of peak)   framework fwd %.3f bwd %.3f ms   out diff %.1e  dy diff %.1e (%d elements beyond 1e-4)" % (
        n, c, r["kernels"]["fwd_ms_median"], r["kernels"]["bwd_ms_median"], r["kernels"]["fwd_fraction_of_peak"],
        r["kernels"]["bwd_fraction_of_peak"], r["framework"]["fwd_ms_median"], r["framework"]["bwd_ms_median"],
        r["max_rel_difference"]["out"], r["max_rel_difference"]["dy"], r["elements_beyond_1e-4"]["dy"]),
        flush=True)
os.makedirs(os.path.join(REPO, "bench_outputs"), exist_ok=True)
json.dump(out, open(os.path.join(REPO, "bench_outputs", "bn_ab.json"), "w"), indent=1)
print(json.dumps(out))
