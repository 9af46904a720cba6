"""Times the two table walks of K4 -- ws_kpconv_gather_bwd_x_gated (one support per wave) and ws_kpconv_gather_bwd_x_packed
(four) -- with HIP events on synthetic strided tables, to set PACK_MEAN_MAX (kpconv.hip): the largest mean in-degree at
which the packed form is still the faster one.

    python3 tools/packed_k4_sweep.py [ns] [ci]          (default 400000 32)

Table of mean in-degree m: nq = ns / 4 queries, query i sits at support 4 i and keeps h = 4 m supports drawn at random
from the 2 h around it, so a support has m incoming pairs on average, binomially spread (some above 16: those take the
single-support path inside the packed kernel).  Supports lie along x one step apart with a jitter of half a radius in y
and z, the radius spans the window; extent = 0.48 radius as in the networks, so one or two kernel points are live per
pair.  The packed entry follows its plan: past the PACK_MEAN_MAX of the build it launches the single-support kernel (the
last column says `none` there), so build with PACK_MEAN_MAX = 32 to time the packed kernel on every row."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from weasal_amd import _lib, ops                                    # noqa: E402
from weasal_amd._lib import check, current_stream, ptr             # noqa: E402

REP = 20


def timed(fn):
    best = 1e9
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REP):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / REP)
    return best


def main():
    ns = int(sys.argv[1]) if len(sys.argv) > 1 else 400000
    ci = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    gen = torch.Generator(device=dev).manual_seed(0)
    nq = ns // 4
    radius = 1.0
    kp = torch.randn(15, 3, device=dev, generator=gen)
    kp = kp / kp.norm(dim=1, keepdim=True) * torch.rand(15, 1, device=dev, generator=gen) ** (1 / 3) * (0.66 * radius)
    print("ns=%d nq=%d ci=%d   ms per launch, best of 5 x %d" % (ns, nq, ci, REP))
    print("%6s %5s %9s %9s %7s  %s" % ("mean", "h", "single", "packed", "ratio", "plan"))
    for mean in (4, 8, 12, 16, 24, 32):
        h = 4 * mean
        step = radius / h
        s = torch.stack([torch.arange(ns, device=dev) * step, (torch.rand(ns, device=dev, generator=gen) - 0.5) * radius,
                         (torch.rand(ns, device=dev, generator=gen) - 0.5) * radius], 1).float().contiguous()
        q = s[::4][:nq].contiguous()
        pick = torch.rand(nq, 2 * h, device=dev, generator=gen).argsort(1)[:, :h]
        inds = (torch.arange(nq, device=dev)[:, None] * 4 - h + pick).clamp_(0, ns - 1).contiguous()
        table = ops.TransposedTable(inds, ns)
        dwf = torch.randn(nq, 15 * ci, device=dev, generator=gen)
        gate = torch.randn(ns, ci, device=dev, generator=gen)
        out = {}
        for name in ("ws_kpconv_gather_bwd_x_gated", "ws_kpconv_gather_bwd_x_packed"):
            dx = torch.empty(ns, ci, device=dev)
            fn = lambda: check(getattr(lib, name)(ptr(q), nq, ptr(s), ns, ptr(inds), h, ptr(table.offsets), ptr(table.pairs), ptr(dwf), ci,
                                                  ptr(kp), 15, None, None, 0.48 * radius, 0, 0, None, ptr(gate), 0.1, ptr(dx),
                                                  current_stream()))
            fn()
            out[name] = (timed(fn), dx)
        (t1, d1), (t4, d4) = out["ws_kpconv_gather_bwd_x_gated"], out["ws_kpconv_gather_bwd_x_packed"]
        assert torch.equal(d1, d4), "the two walks differ at mean in-degree %d" % mean
        buf = C.create_string_buffer(256)
        check(lib.ws_kpconv_gather_bwd_x_packed_variant(nq, ns, h, ci, ptr(dwf), ptr(d4), 0, 0, 0, 0, 0, 0, buf, 256))
        print("%6d %5d %9.4f %9.4f %7.3f  %s" % (mean, h, t1, t4, t4 / t1, buf.value.decode().split("<")[0]), flush=True)


if __name__ == "__main__":
    main()
