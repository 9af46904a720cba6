"""Batch normalisation over the points with the statistics of SEVERAL ranks: the splits both test files walk, their
reference, and the protocol stated rank by rank with five WRONG variants.

No new yardstick: the reference of a split is tests/bn_ref.py on the CONCATENATED rows of all ranks, float64, and the bound is
bn_ref's per-tensor rule

    max |got - ref64|  <=  4 * max |bn_ref in float32 - ref64|  +  1e-6 * max |ref64|

`out`, `dy` and `dresidual` are the ranks' slices laid end to end; save_* and running_* are what a rank holds (every rank must
hold the same); dgamma / dbeta are the SUM over the ranks of what each rank hands to autograd (its local sums).

SPLITS: the smallest shapes at which the two cuts can go wrong -- a rank with one row, ranks of unequal length, an empty
rank (first, and one of eight), three ranks, two rows in all, the scalar column path, eight rows per thread beside a single
row, |mean| / std = 1e3, and a split whose rank 0 rows are shifted by +2 in every column, so that local and global statistics
differ grossly.  Each runs with residual and activation both on and both off.

`protocol(split_id, mutation)` is the operator's protocol in float32 torch, rank by rank, without any collective (the
"gather" is a stack); MUTATIONS are the wrong protocols of the negative control in tests/test_bn_sync_cpu.py.
"""
import functools

import torch

import bn_ref as R

MOMENTUM = 0.02
MUTATIONS = ("local_stats", "local_n_in_dy", "local_n_unbiased", "global_param_grads", "no_mean_difference")
FWD = ("out", "save_mean", "save_rstd", "running_mean", "running_var")
BWD = ("dy", "dgamma", "dbeta", "dresidual")


def _splits():
    base = [("n257-c32-1-256", 257, 32, (1, 256), "normal", 0.0),
            ("n257-c32-128-129", 257, 32, (128, 129), "normal", 0.0),
            ("n257-c32-0-257", 257, 32, (0, 257), "normal", 0.0),
            ("n257-c32-100-100-57", 257, 32, (100, 100, 57), "normal", 0.0),
            ("n2-c1-1-1", 2, 1, (1, 1), "normal", 0.0),
            ("n257-c130-eight-ranks-one-empty", 257, 130, (40, 33, 0, 32, 31, 64, 1, 56), "normal", 0.0),
            ("n65539-c32-65538-1", 65539, 32, (65538, 1), "normal", 0.0),
            ("n1031-c32-bigmean-1000-31", 1031, 32, (1000, 31), "bigmean", 0.0),
            ("n257-c32-128-129-shifted", 257, 32, (128, 129), "normal", 2.0)]
    out = []
    for name, n, c, sizes, data, shift in base:
        assert sum(sizes) == n
        for on in (True, False):
            row = R._row("sync-%s-res%d-act%d" % (name, on, on), n, c, residual=on, act=on, momentum=MOMENTUM, data=data)
            out.append(dict(row, sizes=sizes, shift=shift))
    return out


SPLITS = _splits()
BY_ID = {s["id"]: s for s in SPLITS}
SHIFTED = [s["id"] for s in SPLITS if s["shift"]]
CPU_SPLITS = [s["id"] for s in SPLITS if s["n"] * s["c"] <= 40000]      # what the CPU file's negative control walks


def inputs(sp):
    """bn_ref.inputs of the split's row; the shifted split adds its shift to the rows of rank 0"""
    y, gamma, beta, rm, rv, res, dout = R.inputs(sp)
    if sp["shift"]:
        y = y.clone()
        y[:sp["sizes"][0]] += sp["shift"]
    return y, gamma, beta, rm, rv, res, dout


def bounds(sp):
    """[(begin, end)] of the ranks' rows in the concatenation"""
    out, at = [], 0
    for k in sp["sizes"]:
        out.append((at, at + k))
        at += k
    return out


def tensors(sp):
    return tuple(k for k in FWD + BWD if k != "dresidual" or sp["residual"])


def _evaluate(sp, dtype, given_out=None):
    y, gamma, beta, rm, rv, res, dout = inputs(sp)
    act = 1 if sp["act"] else 0
    f = R.forward(y, gamma, beta, rm, rv, 0, R.EPS, True, MOMENTUM, res, act, R.SLOPE, dtype)
    out = f["out"] if given_out is None else given_out
    b = R.backward(dout, out, y, gamma, f["save_mean"], f["save_rstd"], True, act, R.SLOPE, dtype)
    return {**f, **b}


@functools.lru_cache(maxsize=None)
def case(split_id):
    """(inputs, given_out float32, ref64, err32) of the concatenated rows, as bn_ref.case: every backward gates by the
    float32 restatement's `out`"""
    sp = BY_ID[split_id]
    r32 = _evaluate(sp, torch.float32)
    given = r32["out"].clone()
    r64 = _evaluate(sp, torch.float64, given_out=given)
    names = tensors(sp)
    err32 = {k: float((r32[k].double() - r64[k]).abs().max()) for k in names}
    return inputs(sp), given, {k: r64[k] for k in names + ("num_batches_tracked",)}, err32


def violations(split_id, got):
    _, _, r64, err32 = case(split_id)
    return R.violations(got, r64, err32, [k for k in err32 if k in got])


def merge(records, mutation=None):
    """records [world, 5, c] (n, sum, hi, lo, M2) -> (N [c], sum, M2) of the union: Chan's formula in rank order"""
    cnt, tot, hi, lo, m2 = (records[0, k].clone() for k in range(5))
    for r in range(1, records.shape[0]):
        bn, bs, bh, bl, b2 = (records[r, k] for k in range(5))
        if float(bn[0]) == 0.0:
            continue
        if float(cnt[0]) == 0.0:
            cnt, tot, hi, lo, m2 = (t.clone() for t in (bn, bs, bh, bl, b2))
            continue
        both = cnt + bn
        d, f = (bh - hi) + (bl - lo), bn / both
        m2 = m2 + b2 + (0.0 if mutation == "no_mean_difference" else d * d * (cnt * f))
        tot, lo, cnt = tot + bs, lo + d * f, both
    return cnt, tot, m2


def protocol(split_id, mutation=None):
    """the protocol in float32, rank by rank -> the tensors `violations` takes; rank 0 speaks for save_* and running_*
    (under the correct protocol every rank holds the same), the last rank where rank 0 is empty"""
    sp = BY_ID[split_id]
    (y, gamma, beta, rm, rv, res, dout), given, _, _ = case(split_id)
    c, cuts = sp["c"], bounds(sp)
    records = torch.zeros(len(cuts), 5, c)
    for r, (a, b) in enumerate(cuts):
        if b > a:
            mean = y[a:b].sum(0) / (b - a)
            records[r, 0], records[r, 1], records[r, 2], records[r, 4] = float(b - a), y[a:b].sum(0), mean, ((y[a:b] - mean) ** 2).sum(0)
    total, tot, m2 = merge(records, mutation)
    speaker = 0 if cuts[0][1] > cuts[0][0] else len(cuts) - 1
    got = {k: [] for k in ("out", "dy", "dresidual")}
    got["dgamma"], got["dbeta"] = torch.zeros(c), torch.zeros(c)
    stats, sums = [], torch.zeros(len(cuts), 2, c)
    for r, (a, b) in enumerate(cuts):
        n_here = float(b - a)
        if mutation == "local_stats" and b - a > 1:
            mean, var, n_unb = records[r, 1] / n_here, records[r, 4] / n_here, n_here
        else:
            mean, var = tot / total, m2 / total
            n_unb = n_here if (mutation == "local_n_unbiased" and b - a > 1) else total
        rstd = 1.0 / torch.sqrt(var + R.EPS)
        stats.append((mean, rstd))
        if r == speaker:
            got["save_mean"], got["save_rstd"] = mean, rstd
            got["running_mean"] = (1 - MOMENTUM) * rm + MOMENTUM * mean
            got["running_var"] = (1 - MOMENTUM) * rv + MOMENTUM * (var * (n_unb / (n_unb - 1.0)))
        z = (y[a:b] - mean) * rstd * gamma + beta
        if res is not None:
            z = z + res[a:b]
        got["out"].append(torch.where(z > 0, z, z * R.SLOPE) if sp["act"] else z)
        dz = torch.where(given[a:b] > 0, dout[a:b], dout[a:b] * R.SLOPE) if sp["act"] else dout[a:b]
        sums[r, 0], sums[r, 1] = dz.sum(0), (dz * ((y[a:b] - mean) * rstd)).sum(0)
    s = sums[0].clone()
    for r in range(1, len(cuts)):
        s = s + sums[r]
    for r, (a, b) in enumerate(cuts):
        mean, rstd = stats[r]
        dz = torch.where(given[a:b] > 0, dout[a:b], dout[a:b] * R.SLOPE) if sp["act"] else dout[a:b]
        div = float(b - a) if (mutation == "local_n_in_dy" and b > a) else total
        got["dy"].append(gamma * rstd * (dz - s[0] / div - ((y[a:b] - mean) * rstd) * (s[1] / div)))
        got["dresidual"].append(dz)
        mine = s if mutation == "global_param_grads" else sums[r]
        got["dbeta"], got["dgamma"] = got["dbeta"] + mine[0], got["dgamma"] + mine[1]
    for k in ("out", "dy", "dresidual"):
        got[k] = torch.cat(got[k])
    if not sp["residual"]:
        del got["dresidual"]
    return got


# ------------------------------------------------------------------------------------------------------------------
# rank processes (mp.spawn targets): the operator on a split, and the small 'points' network of tests/test_batchnorm_gpu.py
# ------------------------------------------------------------------------------------------------------------------
def init_rank(rank, world, port):
    """a gloo process group of `world` ranks with a 60 s timeout -> (dist, dp); ranks of a GPU test share the card"""
    import datetime
    import os
    import torch.distributed as dist
    from weasal_amd import dp
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    return dist, dp


def module(sp, device):
    _, gamma, beta, rm, rv, _, _ = inputs(sp)
    bn = torch.nn.BatchNorm1d(sp["c"], momentum=MOMENTUM, eps=R.EPS)
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    return bn.to(device).train()


def op_worker(rank, world, port, split_ids, device, out):
    """ops.batch_norm_act(group=...) on this rank's rows of every split -> out[(split, rank)] = its tensors on the host.  The
    backward gates by the float32 restatement's `out`, as every comparison against bn_ref does: the operator's own output is
    overwritten with it (behind autograd's back) before backward runs"""
    dist, _ = init_rank(rank, world, port)
    from weasal_amd import ops
    group = dist.new_group()
    for sid in split_ids:
        sp = BY_ID[sid]
        assert len(sp["sizes"]) == world
        (y, gamma, beta, rm, rv, res, dout), given, _, _ = case(sid)
        a, b = bounds(sp)[rank]
        bn = module(sp, device)
        yg = y[a:b].to(device).requires_grad_(True)
        rg = res[a:b].to(device).requires_grad_(True) if res is not None else None
        o = ops.batch_norm_act(yg, bn, residual=rg, slope=R.SLOPE if sp["act"] else None, group=group)
        got = {"out": o.detach().clone().cpu()}
        o.data.copy_(given[a:b])
        o.backward(dout[a:b].to(device))
        got.update(dy=yg.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, running_mean=bn.running_mean, running_var=bn.running_var,
                   num_batches_tracked=bn.num_batches_tracked)
        if rg is not None:
            got["dresidual"] = rg.grad
        out[(sid, rank)] = {k: v.detach().cpu().clone() for k, v in got.items()}
    dist.barrier()
    dist.destroy_process_group()


def assemble(split_id, out):
    """the ranks' results of op_worker -> the tensors `violations` takes (rank 0 speaks for the buffers); the buffers and
    num_batches_tracked must be torch.equal across the ranks"""
    sp = BY_ID[split_id]
    ranks = [out[(split_id, r)] for r in range(len(sp["sizes"]))]
    for other in ranks[1:]:
        for k in ("running_mean", "running_var", "num_batches_tracked"):
            assert torch.equal(ranks[0][k], other[k]), "%s: %s differs between ranks" % (split_id, k)
    assert int(ranks[0]["num_batches_tracked"]) == 1
    got = {k: torch.cat([r[k] for r in ranks]) for k in ("out", "dy", "dresidual") if k in ranks[0]}
    got["dgamma"], got["dbeta"] = sum(r["dgamma"] for r in ranks), sum(r["dbeta"] for r in ranks)
    got["running_mean"], got["running_var"] = ranks[0]["running_mean"], ranks[0]["running_var"]
    return got


def single_row_worker(rank, world, port, device, out):
    """one row over all ranks: ValueError on EVERY rank, after the gather, and every rank returns"""
    dist, _ = init_rank(rank, world, port)
    from weasal_amd import ops
    group = dist.new_group()
    sp = BY_ID["sync-n2-c1-1-1-res0-act0"]
    bn = module(sp, device)
    before = (bn.running_mean.clone(), bn.running_var.clone())
    try:
        ops.batch_norm_act(torch.ones(1 if rank == 0 else 0, 1, device=device), bn, group=group)
        out[rank] = "no error"
    except ValueError as e:
        untouched = torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1]) and int(bn.num_batches_tracked) == 0
        out[rank] = "raised" if untouched and "more than 1 value" in str(e) else "raised, but: %s / buffers untouched: %s" % (e, untouched)
    dist.barrier()
    dist.destroy_process_group()


def _rank_batch(device, seed):
    """the golden pyramid of tests/test_batchnorm_gpu.py; seed None: its own features, else features drawn from that seed"""
    from test_batchnorm_gpu import _golden_batch
    batch = _golden_batch()
    if seed is not None:
        g = torch.Generator().manual_seed(seed)
        batch.features = torch.randn(batch.features.shape, generator=g) * 0.5 + 0.1 * seed
    return batch.to(device) if device.type == "cuda" else batch


def _steps(net, batch, cfg, steps, grad_sync, device):
    import contextlib
    from oracle import kpconv_ref
    from weasal_amd import blocks
    from weasal_amd.trainer import make_optimizer, train_step
    rows, names = {}, {m: k for k, m in net.named_modules()}
    plain = blocks.BatchNormBlock.normalise

    def noting(self, y, residual=None, slope=None):      # the rows every BN site sees
        rows[names[self]] = int(y.shape[0])
        return plain(self, y, residual, slope)

    blocks.BatchNormBlock.normalise = noting
    try:
        opt = make_optimizer(net, cfg)
        first = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
        with (kpconv_ref.cpu_reference_mode() if device.type == "cpu" else contextlib.nullcontext()):
            for _ in range(steps):
                _, logits = train_step(net, opt, batch, cfg, grad_sync=grad_sync)
    finally:
        blocks.BatchNormBlock.normalise = plain
    res = {"state": {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, "first": first, "rows": rows,
           "logits": logits.detach().cpu().clone(),
           "grads": {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters() if p.grad is not None}}
    return res


SCENARIOS = ((True, False, 2), (False, False, 2), (True, True, 1))      # (switch on, same batch on every rank, steps)


def net_worker(rank, world, port, device, out):
    """train_steps of the small 'points' network under GradSync on every rank, once per scenario -> out[(sync, same_batch,
    rank)]; sync: dp.sync_batch_norm on or off; same_batch: every rank steps on the golden batch itself, else on features of
    its own"""
    dist, dp = init_rank(rank, world, port)
    from test_batchnorm_gpu import _make_net, _net_config
    for sync, same_batch, steps in SCENARIOS:
        cfg = _net_config("points")
        net = _make_net("points").to(device).train()
        dp.broadcast_parameters(net)
        marked = dp.sync_batch_norm(net) if sync else 0
        live = sum(1 for m in net.modules() if getattr(m, "live", None) and m.live())
        assert live > 5 and marked == (live if sync else 0)
        out[(sync, same_batch, rank)] = _steps(net, _rank_batch(device, None if same_batch else 11 + rank), cfg, steps, dp.GradSync(), device)
    dist.barrier()
    dist.destroy_process_group()


def single_process_step(device):
    """one train_step of the same network on the golden batch, no process group"""
    from test_batchnorm_gpu import _make_net, _net_config
    return _steps(_make_net("points").to(device).train(), _rank_batch(device, None), _net_config("points"), 1, None, device)


def check_networks(out, single):
    """the assertions both test files make on net_worker's results (two ranks)"""
    rel = lambda a, b: float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-30)
    # different batches, switch on: every buffer and parameter equal across the ranks after two steps
    a, b = out[(True, False, 0)]["state"], out[(True, False, 1)]["state"]
    for k in a:
        assert torch.equal(a[k], b[k]), "%s differs between the ranks" % k
        if k.endswith("num_batches_tracked"):
            assert int(a[k]) == 2, k
    assert any(not torch.equal(a[k], out[(True, False, 0)]["first"][k]) for k in a if k.endswith("running_var"))
    # the control: switch off, the running statistics drift apart -- the defect is visible to this test
    a, b = out[(False, False, 0)]["state"], out[(False, False, 1)]["state"]
    drifted = [k for k in a if k.endswith(("running_mean", "running_var")) and not torch.equal(a[k], b[k])]
    assert drifted, "the unsynchronised control shows no drift"
    # the same batch on both ranks: two copies leave mean and biased variance what they were -> the single-process step
    two = out[(True, True, 0)]
    assert rel(two["logits"], single["logits"]) < 1e-4
    assert set(two["grads"]) == set(single["grads"])
    for k, g in single["grads"].items():
        assert rel(two["grads"][k], g) < 1e-4, (k, rel(two["grads"][k], g))
    sites = 0
    for k, v0 in single["first"].items():
        if not k.endswith("running_var"):
            continue
        site = k[:-len(".batch_norm.running_var")]
        n = float(single["rows"][site])
        assert two["rows"][site] == n
        keep = (1.0 - MOMENTUM) * v0.double()
        term_one, term_two = single["state"][k].double() - keep, two["state"][k].double() - keep
        factor = (2 * n / (2 * n - 1)) / (n / (n - 1))
        # the terms are momentum * var * factor, read off float32 buffers of size ~1: 1e-6 absolute is ~8 ulp of those
        assert float((term_two - factor * term_one).abs().max()) <= 1e-4 * float(term_one.abs().max()) + 1e-6, k
        assert rel(two["state"][k[:-3] + "mean"], single["state"][k[:-3] + "mean"]) < 1e-5, k
        sites += 1
    assert sites > 5


def trainer_worker(rank, world, port, out):
    """loop.ModelTrainer applies `batch_norm_sync` when it has a grad_sync and more than one rank, and only then"""
    dist, dp = init_rank(rank, world, port)
    from test_batchnorm_gpu import _make_net, _net_config
    from weasal_amd import loop
    marked = {}
    for key, with_sync in ((True, True), (True, False), (False, True)):
        cfg = _net_config("points")
        if key:
            cfg.batch_norm_sync = True
        net = _make_net("points")
        loop.ModelTrainer(net, cfg, device=torch.device("cpu"), grad_sync=dp.GradSync() if with_sync else None, rank=rank)
        groups = [m.sync_group for m in net.modules() if hasattr(m, "sync_group") and m.live()]
        marked[(key, with_sync)] = sum(g is not None for g in groups), len(groups)
        assert all(g is None or (g is groups[0] and g is not dist.group.WORLD) for g in groups)      # one group, BN's own
    out[rank] = marked
    dist.barrier()
    dist.destroy_process_group()
