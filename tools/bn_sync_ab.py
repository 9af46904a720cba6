"""Batch statistics over all ranks, the whole training step, as a REHEARSAL: two rank processes share one GPU over gloo and
run train_step of DALESPLConfig with `batch_norm_mode = 'points'` under GradSync, each on synthetic DALES batches of its own
(prebuilt: no pyramid work in the timed window), with dp.sync_batch_norm off and on -- two networks alternating step by step
after warm-up.  Wall-clock per step between device synchronisations, and the library's launches per step.

This is functional evidence, not performance: gloo carries every collective through the host, both ranks run on the same
card, and nothing here says what RCCL over xGMI costs.  No pass/fail threshold is attached.

    python tools/bn_sync_ab.py [--ranks 2] [--spheres 4]
"""
import argparse, datetime, json, os, socket, sys, time
import numpy as np, torch
import torch.multiprocessing as mp
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WARMUP, REPS = 3, 10


def _rank(rank, world, port, spheres, out):
    import torch.distributed as dist
    from weasal_amd import _lib, config as wcfg, dp, pyramid, synthetic
    from weasal_amd.architectures import KPFCNN
    from weasal_amd.trainer import make_optimizer, train_step
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    wl = synthetic.WORKLOADS["dales"]
    nets = {}
    for arm in ("local", "synchronised"):
        cfg = wcfg.DALESPLConfig()
        cfg.batch_norm_mode = "points"
        torch.manual_seed(0); np.random.seed(0)
        net = KPFCNN(cfg, np.arange(9), []).to(dev).train()
        dp.broadcast_parameters(net)
        sites = dp.sync_batch_norm(net) if arm == "synchronised" else 0
        nets[arm] = (net, make_optimizer(net, cfg), cfg, dp.GradSync(), sites)
    cfg = nets["local"][2]
    batches = []
    for s in range(2):
        pts, feats, labels, lens = synthetic.make_inputs(10 * rank + s, spheres, wl["points"], wl["radius"], cfg.in_features_dim)
        batches.append(pyramid.build_batch(cfg, torch.from_numpy(pts).to(dev), torch.from_numpy(feats).to(dev),
                                           torch.from_numpy(labels).to(dev), lens, wl["limits"]))
    times, launches = {a: [] for a in nets}, {}
    for it in range(WARMUP + REPS):
        for arm, (net, opt, cfg, sync, _) in nets.items():
            torch.cuda.synchronize(); dist.barrier()
            before, t0 = lib.ws_launch_count(), time.perf_counter()
            train_step(net, opt, batches[it % 2], cfg, grad_sync=sync)
            torch.cuda.synchronize()
            if it >= WARMUP:
                times[arm].append((time.perf_counter() - t0) * 1e3)
            launches[arm] = int(lib.ws_launch_count() - before)
    res = {a: dict(ms_per_step_median=float(np.median(t)), ms_min=float(min(t)), ms_max=float(max(t)), library_launches_per_step=launches[a],
                   bn_sites=nets[a][4]) for a, t in times.items()}
    sd = {k: v.detach().cpu() for k, v in nets["synchronised"][0].state_dict().items()}
    res["rows_level0"] = int(batches[0].points[0].shape[0])
    out[rank] = (res, sd)
    dist.barrier()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--spheres", type=int, default=4, help="spheres per rank and batch")
    args = ap.parse_args()
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = mp.Manager().dict()
    mp.spawn(_rank, args=(args.ranks, port, args.spheres, out), nprocs=args.ranks, join=True)
    res, sd0 = out[0]
    equal = all(all(torch.equal(v, out[r][1][k]) for k, v in sd0.items()) for r in range(1, args.ranks))
    line = dict(tool="bn_sync_ab", backend="gloo, ranks share one GPU (rehearsal)", ranks=args.ranks, spheres_per_rank=args.spheres,
                synchronised_state_equal_across_ranks=equal, **{"rank%d" % r: out[r][0] for r in range(args.ranks)})
    print(json.dumps(line))


if __name__ == "__main__":
    main()
