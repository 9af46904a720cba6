"""GPU: batch statistics over the rows of several ranks -- the cut launch sequence of weasal_amd/csrc/batchnorm.hip
(ws_bn_moments, ws_bn_moments_finish, ws_bn_apply, ws_bn_bwd_sums, ws_bn_bwd_apply) and ops.batch_norm_act(group=...).

Reference, bound and splits: tests/bn_sync_ref.py -- bn_ref in float64 on the concatenated rows of all ranks, the per-tensor
rule 4 * err32 + 1e-6 * max |ref64|; tests/test_bn_sync_cpu.py shows that the bound rejects five wrong protocols.

1. Raw ABI, ONE process.  The finishing entries take gathered arrays, so the ranks of a split are simulated without any
   collective: every slice's record, the records stacked, then finish and apply per slice, each "rank" with running buffers
   of its own.  Per split: the bound; guard words around every buffer (the Guarded / Scratch of tests/test_batchnorm_gpu.py:
   outputs NaN before the call, sentinels around them); every rank ends with the same bits in save_*, running_* and
   num_batches_tracked; a second run gives the same bits; an empty slice launches nothing for its statistics or its sums.
2. With ONE rank the cut sequence gives exactly the bits of ws_bn_fwd / ws_bn_bwd (n2049-c32: merge depth 2; n257-c9: the
   scalar path; n65539-c32: eight rows per thread): the local finish kept the merge order.
3. One row over all ranks: ws_bn_moments_finish writes the count and nothing else.
4. Two fresh rank processes sharing the card over gloo: the operator on two splits, and the small 'points' network of
   tests/test_batchnorm_gpu.py (bn_sync_ref.check_networks: buffers and parameters equal across ranks after two steps on
   different batches, the unsynchronised control drifts, the same batch on both ranks reproduces the single-process step).
"""
import ctypes as C
import socket

import pytest
import torch
import torch.multiprocessing as mp

import bn_ref as R
import bn_sync_ref as S
from test_batchnorm_gpu import Guarded, Scratch, _launches, _lib, raw

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _intact(tag, bufs):
    for name, b in bufs.items():
        assert b.intact(), "%s: guard of %s overwritten" % (tag, name)


def cut_sequence(gpu, ins, sizes, residual, act, given, tag, momentum=S.MOMENTUM):
    """the five entries over the slices of `ins` (bn_ref.inputs layout) as len(sizes) simulated ranks -> the tensors
    bn_sync_ref.violations takes (rank 0 speaks for the buffers, after every rank's were found equal); the backward gates by
    `given`"""
    L = _lib()
    lib = L.lib()
    st = L.current_stream()
    y, gamma, beta, rm, rv, res, dout = ins
    c, world = y.shape[1], len(sizes)
    cuts, at = [], 0
    for k in sizes:
        cuts.append((at, at + k))
        at += k
    act_i = 1 if act else 0
    g_gamma, g_beta = gamma.to(gpu).contiguous(), beta.to(gpu).contiguous()
    vp = lambda t: C.c_void_p(t.data_ptr())
    ranks = []
    gathered = Guarded(gpu, world * 5, c)
    for r, (a, b) in enumerate(cuts):
        n = b - a
        k = dict(n=n, y=Guarded(gpu, n, c, y[a:b]), dout=Guarded(gpu, n, c, dout[a:b]), gate=Guarded(gpu, n, c, given[a:b]),
                 record=Guarded(gpu, 5, c), scratch=Scratch(gpu, lib.ws_bn_scratch_bytes(n, c)))
        if residual:
            k["residual"] = Guarded(gpu, n, c, res[a:b])
        before = _launches(lib)
        L.check(lib.ws_bn_moments(k["y"].ptr, n, c, c, k["record"].ptr, k["scratch"].ptr, st))
        assert _launches(lib) - before == (2 if n else 0), "%s rank %d: launches of ws_bn_moments" % (tag, r)
        torch.cuda.synchronize()
        rec = k["record"].value()
        assert bool(torch.isfinite(rec).all()) and bool((rec[0] == float(n)).all()), tag
        if n == 0:
            assert not rec.any(), tag
        _intact("%s rank %d moments" % (tag, r), {x: k[x] for x in ("y", "record", "scratch")})
        gathered.live[5 * r:5 * r + 5].copy_(rec)
        ranks.append(k)
    for r, k in enumerate(ranks):
        n = k["n"]
        k.update(rm=Guarded(gpu, c, None, rm), rv=Guarded(gpu, c, None, rv), nbt=torch.zeros((1,), dtype=torch.int64, device=gpu),
                 save_mean=Guarded(gpu, c), save_rstd=Guarded(gpu, c), ng=torch.full((3,), -7, dtype=torch.int64, device=gpu),
                 out=Guarded(gpu, n, c))
        L.check(lib.ws_bn_moments_finish(gathered.ptr, world, c, R.EPS, momentum, k["rm"].ptr, k["rv"].ptr, vp(k["nbt"]),
                                         k["save_mean"].ptr, k["save_rstd"].ptr, vp(k["ng"][1:]), st))
        before = _launches(lib)
        L.check(lib.ws_bn_apply(k["y"].ptr, n, c, c, k["save_mean"].ptr, k["save_rstd"].ptr, vp(g_gamma), vp(g_beta),
                                k["residual"].ptr if residual else None, c, act_i, R.SLOPE, k["out"].ptr, c, st))
        assert _launches(lib) - before == (1 if n else 0), tag
        torch.cuda.synchronize()
        assert k["ng"].tolist() == [-7, sum(sizes), -7], (tag, k["ng"].tolist())
        _intact("%s rank %d forward" % (tag, r), {x: v for x, v in k.items() if hasattr(v, "intact")})
        assert gathered.intact(), tag
    sums = Guarded(gpu, world * 2, c)
    for r, k in enumerate(ranks):
        n = k["n"]
        k.update(rec2=Guarded(gpu, 2, c), scratch2=Scratch(gpu, lib.ws_bn_scratch_bytes(n, c)))
        before = _launches(lib)
        L.check(lib.ws_bn_bwd_sums(k["dout"].ptr, c, k["gate"].ptr if act else None, c, k["y"].ptr, c, n, c, k["save_mean"].ptr,
                                   k["save_rstd"].ptr, act_i, R.SLOPE, k["rec2"].ptr, k["scratch2"].ptr, st))
        assert _launches(lib) - before == (2 if n else 0), "%s rank %d: launches of ws_bn_bwd_sums" % (tag, r)
        torch.cuda.synchronize()
        rec = k["rec2"].value()
        assert bool(torch.isfinite(rec).all()) and (n or not rec.any()), tag
        sums.live[2 * r:2 * r + 2].copy_(rec)
    for r, k in enumerate(ranks):
        n = k["n"]
        k.update(dy=Guarded(gpu, n, c), scratch3=Scratch(gpu, lib.ws_bn_scratch_bytes(n, c)))
        if residual:
            k["dres"] = Guarded(gpu, n, c)
        L.check(lib.ws_bn_bwd_apply(k["dout"].ptr, c, k["gate"].ptr if act else None, c, k["y"].ptr, c, n, c, vp(g_gamma),
                                    k["save_mean"].ptr, k["save_rstd"].ptr, sums.ptr, world, vp(k["ng"][1:]), act_i, R.SLOPE,
                                    k["dy"].ptr, c, k["dres"].ptr if residual else None, c, k["scratch3"].ptr, st))
        torch.cuda.synchronize()
        _intact("%s rank %d backward" % (tag, r), {x: v for x, v in k.items() if hasattr(v, "intact")})
        assert sums.intact() and gathered.intact(), tag
        for name in ("out", "dy", "dres", "save_mean", "save_rstd"):
            if name in k:
                assert bool(torch.isfinite(k[name].live).all()), "%s rank %d: %s has non-finite elements (a missed store?)" % (tag, r, name)
    first = ranks[0]
    for r, k in enumerate(ranks[1:], 1):
        for name in ("save_mean", "save_rstd", "rm", "rv"):
            assert torch.equal(first[name].value(), k[name].value()), "%s: %s of rank %d differs from rank 0's" % (tag, name, r)
        assert int(k["nbt"]) == int(first["nbt"])
    got = {"out": torch.cat([k["out"].value() for k in ranks]), "dy": torch.cat([k["dy"].value() for k in ranks]),
           "save_mean": first["save_mean"].value(), "save_rstd": first["save_rstd"].value(), "running_mean": first["rm"].value(),
           "running_var": first["rv"].value(), "num_batches_tracked": int(first["nbt"]),
           "dbeta": sum(k["rec2"].value()[0] for k in ranks), "dgamma": sum(k["rec2"].value()[1] for k in ranks)}
    if residual:
        got["dresidual"] = torch.cat([k["dres"].value() for k in ranks])
    return got


@pytest.mark.parametrize("split_id", [s["id"] for s in S.SPLITS])
def test_cut_sequence_on_simulated_ranks(gpu, split_id):
    sp = S.BY_ID[split_id]
    ins, given, r64, err32 = S.case(split_id)
    first = cut_sequence(gpu, ins, sp["sizes"], sp["residual"], sp["act"], given, split_id)
    for key in err32:
        err = float((first[key].double().cpu() - r64[key]).abs().max())
        print("split %-52s %-12s kernel %.3e  float32 restatement %.3e  ratio %.3f" % (
            split_id, key, err, err32[key], err / err32[key] if err32[key] else float("inf") if err else 0.0))
    bad = S.violations(split_id, first)
    assert not bad, (split_id, bad)
    assert first["num_batches_tracked"] == 1
    again = cut_sequence(gpu, ins, sp["sizes"], sp["residual"], sp["act"], given, split_id + " again")
    for key, v in first.items():
        same = torch.equal(v, again[key]) if isinstance(v, torch.Tensor) else v == again[key]
        assert same, "%s: %s differs run to run" % (split_id, key)


@pytest.mark.parametrize("row_id", ["n2049-c32", "n257-c9", "n65539-c32-eight-rows-per-thread"])
def test_one_rank_gives_the_bits_of_the_uncut_entries(gpu, row_id):
    row = R.BY_ID[row_id]
    ins, given, _, _ = R.case(row_id)
    want = raw(gpu, row, row_id, given)
    got = cut_sequence(gpu, ins, (row["n"],), row["residual"], row["act"], given, row_id + " cut", momentum=row["momentum"])
    for key, v in got.items():
        same = torch.equal(v, want[key]) if isinstance(v, torch.Tensor) else v == want[key]
        assert same, "%s: %s of the cut sequence differs from ws_bn_fwd / ws_bn_bwd" % (row_id, key)
    assert set(want) <= set(got)


def test_one_row_over_all_ranks_writes_the_count_alone(gpu):
    L = _lib()
    lib = L.lib()
    c = 8
    for sizes in ((1, 0), (0, 0)):
        gathered = Guarded(gpu, 10, c, torch.zeros(10, c))
        gathered.live[0] = float(sizes[0])
        gathered.live[1:5] = 0.5
        rm, rv, sm, sr = (Guarded(gpu, c) for _ in range(4))
        nbt = torch.zeros((1,), dtype=torch.int64, device=gpu)
        ng = torch.full((1,), -7, dtype=torch.int64, device=gpu)
        L.check(lib.ws_bn_moments_finish(gathered.ptr, 2, c, R.EPS, 0.1, rm.ptr, rv.ptr, C.c_void_p(nbt.data_ptr()), sm.ptr, sr.ptr,
                                         C.c_void_p(ng.data_ptr()), L.current_stream()))
        torch.cuda.synchronize()
        assert int(ng) == sum(sizes) and int(nbt) == 0
        assert all(bool(torch.isnan(b.live).all()) and b.intact() for b in (rm, rv, sm, sr))


@pytest.mark.timeout(300)
def test_operator_on_two_ranks_sharing_the_card(gpu):
    ids = [s["id"] for s in S.SPLITS if s["sizes"] in ((128, 129), (0, 257)) and not s["shift"]]
    assert len(ids) == 4
    out = mp.Manager().dict()
    mp.spawn(S.op_worker, args=(2, _free_port(), ids, gpu, out), nprocs=2, join=True)      # fresh children
    for sid in ids:
        bad = S.violations(sid, S.assemble(sid, out))
        assert not bad, (sid, bad)


@pytest.mark.timeout(120)
def test_one_row_over_two_ranks_raises_on_both(gpu):
    out = mp.Manager().dict()
    mp.spawn(S.single_row_worker, args=(2, _free_port(), gpu, out), nprocs=2, join=True)
    assert dict(out) == {0: "raised", 1: "raised"}


@pytest.mark.timeout(600)
def test_network_on_two_ranks_sharing_the_card(gpu):
    out = mp.Manager().dict()
    mp.spawn(S.net_worker, args=(2, _free_port(), gpu, out), nprocs=2, join=True)      # fresh children, every scenario
    S.check_networks(dict(out), S.single_process_step(gpu))
