#!/usr/bin/env python3
"""What the training loop costs over the bare step: the benchmark's default DALES-shaped workload, two loops in ONE process,
alternating, RUNS runs of STEPS steps each after WARMUP warm-up steps:
  (a) the bare loop of bench.py: next(prefetcher), trainer.train_step, InFlightLimiter.tick; finish() at the end
  (b) loop.ModelTrainer.train with saving off (one epoch of STEPS steps): the same step plus ops.step_stats, an event per
      step, and the one flush at the end of the epoch
Both drive the same network, optimizer and prefetcher.  Prints ms per step of every run, the means, (a)'s max - min spread,
and the HIP-event time of the statistics launches alone on logits of the workload's size.

    python tools/loop_overhead.py [--out profiles/NAME.txt]
"""
import argparse
import itertools
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RUNS, STEPS, WARMUP = 5, 20, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from weasal_amd import config as wcfg, ops, synthetic
    from weasal_amd.architectures import KPFCNN
    from weasal_amd.loop import ModelTrainer, StepLog
    from weasal_amd.prefetch import PyramidPrefetcher
    from weasal_amd.trainer import InFlightLimiter, freeze_gc, train_step
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    wl = synthetic.WORKLOADS["dales"]
    cfg = getattr(wcfg, wl["config"])()
    cfg.saving, cfg.max_epoch, cfg.epoch_steps = False, 1, STEPS
    np.random.seed(1234)
    torch.manual_seed(1234)
    net = KPFCNN(cfg, np.arange(9), []).to(dev).train()
    inputs = []
    for i in range(4):
        pts, feats, labels, lens = synthetic.make_inputs(i, wl["spheres"], wl["points"], wl["radius"], cfg.in_features_dim)
        inputs.append((torch.from_numpy(pts).to(dev), torch.from_numpy(feats).to(dev), torch.from_numpy(labels).to(dev), lens))
    pf = PyramidPrefetcher(cfg, itertools.cycle(inputs), wl["limits"], depth=2, device=dev)
    trainer = ModelTrainer(net, cfg, device=dev)
    trainer.console = False
    opt = trainer.optimizer

    def bare(steps):
        limiter = InFlightLimiter()
        for _ in range(steps):
            batch = next(pf)
            train_step(net, opt, batch, cfg, epoch=0)
            limiter.tick(batch)
        limiter.finish()

    def looped(steps):
        trainer.epoch = 0
        trainer.train(net, lambda epoch: itertools.islice(pf, steps))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(STEPS)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / STEPS

    lines = []
    try:
        bare(12)
        torch.cuda.synchronize()
        freeze_gc()
        bare(WARMUP)
        sys.stdout = open(os.devnull, "w")              # ('Finished Training' of every run)
        looped(WARMUP)
        a, b = [], []
        for _ in range(RUNS):
            a.append(timed(bare))
            b.append(timed(looped))
        sys.stdout = sys.__stdout__
        assert trainer.log.host_reads == 1
        # the statistics launches alone
        n = int(wl["spheres"] * wl["points"])
        logits = torch.randn((n, 9), device=dev)
        labels = torch.randint(0, 9, (n,), device=dev)
        one = torch.ones(1, device=dev)
        log = StepLog(64, dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(5):
            ops.step_stats(log.ring, 0, logits, labels, None, one, one, one)
        ev[0].record()
        for r in range(50):
            ops.step_stats(log.ring, r, logits, labels, None, one, one, one)
        ev[1].record()
        torch.cuda.synchronize()
        kernel_us = 1e3 * ev[0].elapsed_time(ev[1]) / 50
    finally:
        sys.stdout = sys.__stdout__
        pf.close()
    spread = max(a) - min(a)
    lines.append("workload: %s; %d runs of %d steps after %d warm-up, alternating (a), (b); ms per step" % (wl["name"], RUNS, STEPS, WARMUP))
    lines.append("(a) bare train_step + InFlightLimiter : " + " ".join("%.3f" % v for v in a) + "   mean %.3f  max - min %.3f" % (np.mean(a), spread))
    lines.append("(b) ModelTrainer.train, saving off     : " + " ".join("%.3f" % v for v in b) + "   mean %.3f" % np.mean(b))
    lines.append("mean (b) - mean (a) = %+.3f ms per step; inside (a)'s spread above its mean: %s"
                 % (np.mean(b) - np.mean(a), "yes" if np.mean(b) <= np.mean(a) + spread else "NO"))
    lines.append("ws_step_stats alone on [%d, 9] logits (both launches, HIP events over 50 calls): %.1f us per call" % (n, kernel_us))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
