"""GPU: every launch branch of weasal_amd/csrc/batchnorm.hip against tests/bn_ref.py in float64.

The rows are bn_ref.ROWS; tests/test_batchnorm_cpu.py shows which branch of the plan each one reaches and that the bound
below rejects seven kinds of wrong kernel.

1. The C entries are called directly (ctypes), so every buffer is the test's own.
2. Every output (out, save_mean, save_rstd, dy, dresidual, dgamma, dbeta) is NaN in its live region before the call and the
   scratch is NaN throughout: a store the kernels miss, or a scratch word they read before writing it, comes back as NaN.
   Every buffer carries 64 guard rows past row N -- and, where the pitch is above C, the columns past C of every row --
   the scratch 256 guard bytes past ws_bn_scratch_bytes, holding a finite sentinel that must come back bit-unchanged.
3. The bound is the project's rule for kernels that replace a float32 torch path, per tensor:

       max |kernel - ref64|  <=  4 * max |bn_ref in float32 on the CPU - ref64|  +  1e-6 * max |ref64|

   num_batches_tracked is exact.  The backward of the kernel and of both references gate by the SAME float32 `out` tensor
   (the float32 restatement's), so no activation-kink flip exists; no element is masked or skipped.
4. Every row prints kernel error, yardstick and ratio per tensor.
5. Every row runs twice into fresh poisoned buffers: the two results are torch.equal.

Beside the table: N = 0 (status 0, nothing launched, nothing touched), training with one row (refused, nothing written),
the ops wrapper with autograd against the raw calls (same bits), two consecutive training calls through the wrapper, a
two-step train_step of a small 'points' KPFCNN against the same network under oracle.kpconv_ref.cpu_reference_mode (1e-4,
the project's float32 rule), and reference mode bit-identical with WEASAL_BN_KERNELS unset and 0 (a child process).

Largest ratio kernel error / float32-restatement error per tensor over the rows, MI355X:

    save_mean 8.09 (n257-c1)   dgamma 4.90 (n700003-c3-chunk-cap)   save_rstd 3.04 (n63-c3)   dbeta 2.64 (n257-c9-bigmean-eval)
    out 1.98 (n1-c32-eval)     running_var 1.77   dy 1.56   running_mean 1.28   dresidual 1.00

The two above 4 are inside through the 1e-6 * max |ref64| term (save_mean of a unit-normal column: 1.3e-8 absolute).  The
first version of the kernels kept a partial mean as ONE float and missed save_rstd at |mean| / std = 1e3 by a ratio of 29.5
(n1031-c32-bigmean); a second kept it as hi + lo and reported hi + lo as the mean, and missed save_mean on nine unit-normal
rows by up to 1.8e-7 absolute.  The kernels changed both times, the bound and the rows did not.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bn_ref as R

pytestmark = pytest.mark.gpu

GUARD_ROWS = 64
SCRATCH_GUARD = 256             # bytes
SENTINEL = 12345.678            # finite, not a value any row produces
_BITS = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32).item()


def _lib():
    from weasal_amd import _lib as L
    return L


class Guarded:
    """[rows + 64, ld] on the device, `offset` floats into its allocation: the live [rows, width] block holds `src` or NaN,
    everything else -- guard rows, the columns past `width`, the floats in front -- the sentinel.  width None: a vector."""

    def __init__(self, gpu, rows, width=None, src=None, ld=None, offset=0):
        vector = width is None
        width = 1 if vector else width
        ld = ld or width
        self.flat = torch.full(((rows + GUARD_ROWS) * ld + offset,), SENTINEL, dtype=torch.float32, device=gpu)
        self.full = self.flat[offset:].view(rows + GUARD_ROWS, ld)
        self.live = self.full[:rows, :width]
        self.ld = ld
        if src is None:
            self.live.fill_(float("nan"))
        else:
            self.live.copy_(src.to(gpu).view(rows, width))
        self.vector = vector

    @property
    def ptr(self):
        return C.c_void_p(self.full.data_ptr())

    def value(self):
        v = self.live.clone()
        return v.view(-1) if self.vector else v

    def intact(self):
        rest = self.flat.clone()
        rest[self.flat.numel() - self.full.numel():].view(self.full.shape)[:self.live.shape[0], :self.live.shape[1]] = SENTINEL
        return bool((rest.view(torch.int32) == _BITS).all())


class Scratch:
    def __init__(self, gpu, nbytes):
        assert nbytes % 4 == 0
        self.words = nbytes // 4
        self.buf = torch.full((self.words + SCRATCH_GUARD // 4,), float("nan"), dtype=torch.float32, device=gpu)
        self.buf[self.words:] = SENTINEL

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr())

    def intact(self):
        return bool((self.buf[self.words:].view(torch.int32) == _BITS).all())


def _launches(lib):
    return C.c_longlong.in_dll(lib, "ws_launch_counter").value


def raw(gpu, row, tag, given=None, expect=0):
    """ws_bn_fwd + ws_bn_bwd of a row on guarded, poisoned buffers -> {tensor: value}; the backward gates by `given` (None:
    the kernel's own output).  expect != 0: the forward must return that status and write nothing."""
    L = _lib()
    lib = L.lib()
    y, gamma, beta, rm, rv, res, dout = R.inputs(row)
    n, c, ld = row["n"], row["c"], row["c"] + row["pad"]
    off = lambda name: 1 if row["off"] == name else 0
    training, act = (1 if row["training"] else 0), (1 if row["act"] else 0)
    st = L.current_stream()
    dev = lambda t: t.to(gpu).contiguous()
    ins = {"y": Guarded(gpu, n, c, y, ld, off("y")), "dout": Guarded(gpu, n, c, dout, ld, off("dout"))}
    if res is not None:
        ins["residual"] = Guarded(gpu, n, c, res, ld, off("residual"))
    g_gamma, g_beta = dev(gamma), dev(beta)
    st_rm, st_rv = Guarded(gpu, c, None, rm), Guarded(gpu, c, None, rv)
    nbt = torch.zeros((1,), dtype=torch.int64, device=gpu)
    fwd = {"out": Guarded(gpu, n, c, None, ld, off("out"))}
    if training:
        fwd.update(save_mean=Guarded(gpu, c), save_rstd=Guarded(gpu, c))
    nbytes = lib.ws_bn_scratch_bytes(n, c)
    assert nbytes >= 0
    scratch = Scratch(gpu, nbytes)
    before = _launches(lib)
    rc = lib.ws_bn_fwd(ins["y"].ptr, n, c, ld, C.c_void_p(g_gamma.data_ptr()), C.c_void_p(g_beta.data_ptr()), R.EPS, training,
                       row["momentum"], st_rm.ptr, st_rv.ptr, C.c_void_p(nbt.data_ptr()), ins["residual"].ptr if res is not None else None,
                       ld, act, R.SLOPE, fwd["out"].ptr, ld, fwd["save_mean"].ptr if training else None,
                       fwd["save_rstd"].ptr if training else None, scratch.ptr if training else None, st)
    torch.cuda.synchronize()
    everything = {**ins, **fwd, "running_mean": st_rm, "running_var": st_rv, "scratch": scratch}
    if expect or n == 0:
        assert rc == expect, (tag, rc, lib.ws_last_error())
        assert _launches(lib) == before, "%s: something was launched" % tag
        assert all(b.intact() for b in everything.values()) and int(nbt) == 0
        assert all(bool(torch.isnan(b.live).all()) for b in fwd.values()), "%s: a call that had nothing to do wrote" % tag
        assert torch.equal(st_rm.value().cpu(), rm) and torch.equal(st_rv.value().cpu(), rv)
        return None
    L.check(rc)
    assert _launches(lib) - before == (3 if training else 1), tag
    for name, b in everything.items():
        assert b.intact(), "%s forward: guard of %s overwritten" % (tag, name)
    res_out = {}
    for name, b in fwd.items():
        assert bool(torch.isfinite(b.live).all()), "%s: %s has non-finite elements (a missed store?)" % (tag, name)
        res_out[name] = b.value()
    res_out["running_mean"], res_out["running_var"], res_out["num_batches_tracked"] = st_rm.value(), st_rv.value(), int(nbt)
    if not training:
        assert torch.equal(res_out["running_mean"].cpu(), rm) and torch.equal(res_out["running_var"].cpu(), rv) and int(nbt) == 0, tag

    gate = Guarded(gpu, n, c, res_out["out"] if given is None else given, ld, off("out"))
    bwd = {"dy": Guarded(gpu, n, c, None, ld, off("dy")), "dgamma": Guarded(gpu, c), "dbeta": Guarded(gpu, c)}
    if row["dres"]:
        bwd["dresidual"] = Guarded(gpu, n, c, None, ld, off("dresidual"))
    scratch = Scratch(gpu, nbytes)
    L.check(lib.ws_bn_bwd(ins["dout"].ptr, ld, gate.ptr if act else None, ld, ins["y"].ptr, ld, n, c, C.c_void_p(g_gamma.data_ptr()),
                          fwd["save_mean"].ptr if training else None, fwd["save_rstd"].ptr if training else None,
                          None if training else st_rm.ptr, None if training else st_rv.ptr, R.EPS, training, act, R.SLOPE,
                          bwd["dy"].ptr, ld, bwd["dresidual"].ptr if row["dres"] else None, ld, bwd["dgamma"].ptr, bwd["dbeta"].ptr,
                          scratch.ptr, st))
    torch.cuda.synchronize()
    for name, b in {**everything, **bwd, "gate": gate, "scratch": scratch}.items():
        assert b.intact(), "%s backward: guard of %s overwritten" % (tag, name)
    for name, b in bwd.items():
        assert bool(torch.isfinite(b.live).all()), "%s: %s has non-finite elements (a missed store?)" % (tag, name)
        res_out[name] = b.value()
    return res_out


def _check(tag, row, got, r64, err32):
    names = tuple(k for k in R.tensors(row) if k in got)
    for key in names:
        ref = r64[key]
        err = float((got[key].double().cpu() - ref).abs().max()) if ref.numel() else 0.0
        print("branch %-42s %-12s kernel %.3e  float32 restatement %.3e  ratio %.3f  max|ref| %.3e" % (
            tag, key, err, err32[key], err / err32[key] if err32[key] else float("inf") if err else 0.0, float(ref.abs().max())))
    bad = R.violations(got, r64, err32, names)
    assert not bad, (tag, bad)
    assert got["num_batches_tracked"] == r64["num_batches_tracked"], tag


@pytest.mark.parametrize("row_id", [r["id"] for r in R.ROWS])
def test_batchnorm_branch(gpu, row_id):
    row = R.BY_ID[row_id]
    _, given, r64, err32 = R.case(row_id)
    first = raw(gpu, row, row_id, given)
    if row["residual"] and not row["dres"]:
        assert "dresidual" not in first
    _check(row_id, row, first, r64, err32)
    again = raw(gpu, row, row_id + " again", given)
    for key, v in first.items():
        same = torch.equal(v, again[key]) if isinstance(v, torch.Tensor) else v == again[key]
        assert same, "%s: %s differs run to run" % (row_id, key)


def test_zero_rows_and_single_training_row(gpu):
    assert raw(gpu, R._row("n0-c32", 0, 32, residual=True, act=True), "n0") is None
    assert raw(gpu, R._row("n0-c9-eval", 0, 9, training=False), "n0 eval") is None
    assert raw(gpu, R._row("n1-c32-train", 1, 32, act=True), "n1 training", expect=1) is None
    # the backward of nothing: zero column sums, no kernel
    L = _lib()
    lib = L.lib()
    dg, db = Guarded(gpu, 8), Guarded(gpu, 8)
    before = _launches(lib)
    p = C.c_void_p(dg.ptr.value)
    L.check(lib.ws_bn_bwd(None, 8, None, 8, None, 8, 0, 8, p, None, None, None, None, R.EPS, 1, 1, R.SLOPE, None, 8, None, 8, dg.ptr,
                          db.ptr, None, L.current_stream()))
    torch.cuda.synchronize()
    assert _launches(lib) == before and not dg.value().any() and not db.value().any() and dg.intact() and db.intact()


def _module(gpu, row, training=True):
    _, gamma, beta, rm, rv, _, _ = R.inputs(row)
    bn = torch.nn.BatchNorm1d(row["c"], momentum=row["momentum"], eps=R.EPS)
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    return bn.to(gpu).train(training)


@pytest.mark.parametrize("row_id", ["n257-c32-train-res1-act1", "n257-c32-eval-res1-act1", "n257-c9", "n2049-c32"])
def test_ops_path_gives_the_bits_of_the_raw_calls(gpu, row_id):
    from weasal_amd import ops
    row = R.BY_ID[row_id]
    y, _, _, _, _, res, dout = R.inputs(row)
    want = raw(gpu, row, row_id)                       # (the backward gates by the kernel's own output, as autograd does)
    bn = _module(gpu, row, row["training"])
    yg = y.to(gpu).requires_grad_(True)
    rg = res.to(gpu).requires_grad_(True) if res is not None else None
    out = ops.batch_norm_act(yg, bn, residual=rg, slope=R.SLOPE if row["act"] else None)
    out.backward(dout.to(gpu))
    got = {"out": out.detach(), "dy": yg.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad, "running_mean": bn.running_mean,
           "running_var": bn.running_var}
    if rg is not None:
        got["dresidual"] = rg.grad
    for key, v in got.items():
        assert torch.equal(v, want[key]), "%s: %s differs from the raw call in %d elements" % (row_id, key, int((v != want[key]).sum()))
    assert int(bn.num_batches_tracked) == want["num_batches_tracked"]
    with pytest.raises(ValueError):
        ops.batch_norm_act(torch.zeros(1, row["c"], device=gpu), _module(gpu, row, True))
    with pytest.raises(ValueError):
        ops.batch_norm_act(torch.zeros(4, row["c"], device=gpu, dtype=torch.bfloat16), bn)
    bn.momentum = None
    with pytest.raises(ValueError):
        ops.batch_norm_act(yg.detach(), bn)
    empty = ops.batch_norm_act(torch.zeros(0, row["c"], device=gpu), _module(gpu, row, True))
    assert empty.shape == (0, row["c"])


def test_two_training_calls_update_the_running_statistics(gpu):
    from weasal_amd import ops
    row = R.BY_ID["n1031-c32-negmean"]
    _, gamma, beta, rm, rv, _, _ = R.inputs(row)
    bn = _module(gpu, row)
    g = torch.Generator().manual_seed(11)
    state = {t: {"rm": rm.to(t), "rv": rv.to(t), "nbt": 0} for t in (torch.float32, torch.float64)}
    for call in range(2):
        y = torch.randn(row["n"], row["c"], generator=g) * (3.0 + call) - 300.0 * call
        bn.momentum = 0.02 if call == 0 else 0.3                     # read at each call
        ops.batch_norm_act(y.to(gpu), bn, slope=0.1)
        for t, s in state.items():
            f = R.forward(y, gamma, beta, s["rm"], s["rv"], s["nbt"], R.EPS, True, bn.momentum, None, 1, 0.1, t)
            s["rm"], s["rv"], s["nbt"] = f["running_mean"], f["running_var"], f["num_batches_tracked"]
    s32, s64 = state[torch.float32], state[torch.float64]
    for key, buf in (("rm", bn.running_mean), ("rv", bn.running_var)):
        err, yard = float((buf.double().cpu() - s64[key]).abs().max()), float((s32[key].double() - s64[key]).abs().max())
        print("two calls %-3s kernel %.3e  float32 restatement %.3e  ratio %.3f" % (key, err, yard, err / yard if yard else 0.0))
        assert err <= 4 * yard + 1e-6 * float(s64[key].abs().max()), key
    assert int(bn.num_batches_tracked) == 2


# ------------------------------------------------------------------------------------------------------------------
# the network
# ------------------------------------------------------------------------------------------------------------------
def _net_config(mode):
    from weasal_amd.config import Config

    class Cfg(Config):
        architecture = ['simple', 'resnetb', 'resnetb_strided', 'resnetb', 'resnetb_strided', 'resnetb',
                        'nearest_upsample', 'unary', 'nearest_upsample', 'unary']
        first_subsampling_dl = 0.24
        deform_radius = 6.0
        first_features_dim = 16                 # widths 16, 32, 64
        in_features_dim = 4
        batch_norm_momentum = 0.02
        repulse_extent = 1.2
        learning_rate = 0.01
        momentum = 0.98
        dropout = 0
        saving = False
    cfg = Cfg()
    if mode == 'points':
        cfg.batch_norm_mode = 'points'
    return cfg


def _golden_batch():
    from conftest import golden
    from weasal_amd import pyramid
    g7 = golden("g7_pyramid.npz")
    L = 5
    flat = ([g7["points_%d" % l] for l in range(L)] + [g7["neighbors_%d" % l] for l in range(L)]
            + [g7["pools_%d" % l] for l in range(L)] + [g7["upsamples_%d" % l] for l in range(L)]
            + [g7["lengths_%d" % l] for l in range(L)] + [g7["features"], g7["labels"]])
    return pyramid.PyramidBatch([torch.from_numpy(np.ascontiguousarray(a)) for a in flat])


def _make_net(mode):
    from weasal_amd.architectures import KPFCNN
    np.random.seed(0)
    torch.manual_seed(0)
    net = KPFCNN(_net_config(mode), np.arange(9), [])
    with torch.no_grad():                     # BN parameters and buffers off their initial 1 / 0, so that a swap would show
        g = torch.Generator().manual_seed(3)
        for name, t in list(net.named_parameters()) + list(net.named_buffers()):
            if name.endswith("batch_norm.weight"):
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
            elif name.endswith("batch_norm.bias") or name.endswith("running_mean"):
                t.copy_(torch.randn(t.shape, generator=g) * 0.1)
            elif name.endswith("running_var"):
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
    return net


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def test_points_network_two_steps_vs_cpu_reference(gpu):
    from oracle import kpconv_ref
    from weasal_amd import fused
    from weasal_amd.trainer import make_optimizer, train_step
    cfg = _net_config('points')
    net_g, net_c = _make_net('points'), _make_net('points')
    net_c.load_state_dict(net_g.state_dict())
    net_g.to(gpu).train()
    net_c.train()
    batch_g, batch_c = _golden_batch().to(gpu), _golden_batch()
    opt_g, opt_c = make_optimizer(net_g, cfg), make_optimizer(net_c, cfg)
    hits = fused.gate_link_hits, fused.skip_slot_hits
    for step in range(2):
        loss_g, out_g = train_step(net_g, opt_g, batch_g, cfg)
        with kpconv_ref.cpu_reference_mode():
            loss_c, out_c = train_step(net_c, opt_c, batch_c, cfg)
        print("step %d  logits %.3e  loss %.3e" % (step, _rel(out_g, out_c), abs(float(loss_g.detach()) - float(loss_c.detach()))))
        assert _rel(out_g, out_c) < 1e-4 and abs(float(loss_g.detach()) - float(loss_c.detach())) < 1e-4 * max(abs(float(loss_c.detach())), 1.0)
    assert (fused.gate_link_hits, fused.skip_slot_hits) == hits            # every fused route declined
    sd_g, sd_c = net_g.state_dict(), net_c.state_dict()
    worst = ("", 0.0)
    for k, v in sd_c.items():
        if k.endswith("num_batches_tracked"):
            assert int(sd_g[k]) == int(v) == 2, k
            continue
        e = _rel(sd_g[k], v)
        worst = max(worst, (k, e), key=lambda kv: kv[1])
        assert e < 1e-4, (k, e)
    print("worst tensor after two steps: %s %.3e" % worst)
    moved = [k for k in sd_c if k.endswith("batch_norm.weight")]
    fresh = _make_net('points').state_dict()
    assert moved and all(not torch.equal(sd_c[k], fresh[k]) for k in moved)       # gamma trains
    # evaluation with the running statistics
    net_g.eval(), net_c.eval()
    with torch.no_grad():
        ev_g = net_g(batch_g, cfg)
        with kpconv_ref.cpu_reference_mode():
            ev_c = net_c(batch_c, cfg)
    assert _rel(ev_g, ev_c) < 1e-4


def _reference_mode_logits(gpu):
    cfg = _net_config('reference')
    net = _make_net('reference').to(gpu).train()
    batch = _golden_batch().to(gpu)
    out = net(batch, cfg)
    out.square().mean().backward()
    grads = torch.cat([p.grad.reshape(-1) for p in net.parameters() if p.grad is not None])
    return out.detach().cpu(), grads.cpu()


def test_reference_mode_is_untouched_by_the_switch(gpu, tmp_path):
    """reference mode in this process (WEASAL_BN_KERNELS unset) and in a fresh one with WEASAL_BN_KERNELS=0: the same bits"""
    out, grads = _reference_mode_logits(gpu)
    path = str(tmp_path / "reference_mode.pt")
    env = {k: v for k, v in os.environ.items() if k != "WEASAL_BN_KERNELS"}
    proc = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(env, WEASAL_BN_KERNELS="0"), capture_output=True,
                          text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    other = torch.load(path)
    assert torch.equal(out, other["out"]) and torch.equal(grads, other["grads"])
    net = _make_net('reference')
    assert all(p.grad is None for k, p in net.named_parameters() if "batch_norm" in k)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from weasal_amd import ops as _ops
    assert not _ops.BN_KERNELS
    _out, _grads = _reference_mode_logits(torch.device("cuda:0"))
    torch.save({"out": _out, "grads": _grads}, sys.argv[1])
