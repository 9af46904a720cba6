"""GPU: every launch branch of weasal_amd/csrc/attention.hip against tests/att_ref.py in float64.

The rows are SPATIAL_ROWS / CHANNEL_ROWS of tests/att_branch_ref.py; tests/test_attention_branches_cpu.py shows which
instantiation, output-tile masking, dv slice count, dv chunk walk, sphere structure and softmax lane layout each one reaches,
and that the bound below rejects eleven kinds of wrong kernel.

1. The C entries are called directly (ctypes), so every buffer is the test's own.
2. Every output (att, xn, lse, d_q, d_k, d_v; a, out, d_x1, d_x2, d_value) is NaN in its live region before the call and the
   scratch is NaN throughout: a store the kernels miss, or a scratch word they read before writing it, comes back as NaN
   (outputs from torch.empty can hand back a freed buffer that already holds the right values).  Every buffer carries 64
   guard rows past row N, the scratch 256 guard bytes past scratch_bytes, holding a finite sentinel that must come back
   bit-unchanged.
3. The bound is the project's rule for kernels that replace a float32 torch path, per tensor and row:

       max |kernel - ref64|  <=  4 * max |att_ref in float32 on the CPU - ref64|  +  1e-6 * max |ref64|

4. Every row prints kernel error, yardstick and ratio per tensor.
5. Every row runs twice into fresh poisoned buffers: the two results are torch.equal.

Beside the tables: the d_att == NULL / d_xn == NULL halves of the backward pre-pass against explicit zero tensors, q and k
one float off 16-byte alignment (same bits; a v that is one float off is refused), the ops wrappers with autograd against
the raw calls (same bits), and all-empty calls (status 0, nothing launched).

Largest ratio kernel error / float32-loop error per tensor over the rows, MI355X (every row was inside the bound at its
first run; no kernel changed):

    sphere form    att 1.28 (dq48-dv64-cap-peaked)      xn 3.19 (dq24-dv128-cap-ramp)      dv 3.30 (dq8-dv192-empties-peaked)
                   dq  6.69, dk 6.30 (dq8-dv128-edges-mild);  2.60 / 2.42 over all other rows
    channel form   out 1.02, dvalue 1.10 (channel-c12-mm1-cap)   dx1 1.46 (channel-c64-mm1-edges)   dx2 1.41 (elevation-c96-mm0-edges)

dq8-dv128-edges-mild is the one row that needs the 1e-6 * max |ref64| term: dq 1.027e-6 against 4 * 1.536e-7 + 4.861e-7,
dk 9.721e-7 against 4 * 1.542e-7 + 6.595e-7.  All of it sits in the sphere of ONE row, whose dQ and dK are zero
(softmax of one energy is constant): the loop's softmax backward gives P (dP - P dP) = 0 exactly, the kernels form
dS = P (dO V^T - D) with D = rowsum(dO o att) from the pre-pass and dO V^T on the matrix core -- the same 128 products of
magnitude ~4 summed in two orders, one ulp of 4 apart.  In the other spheres of that row the ratio is 1.0 - 2.4.
"""
import ctypes as C
import math

import pytest
import torch

import att_branch_ref as R

pytestmark = pytest.mark.gpu

GUARD_ROWS = 64
SCRATCH_GUARD = 256             # bytes
SENTINEL = 12345.678            # finite, not a value any row produces


def _lib():
    from weasal_amd import _lib as L
    return L


class Guarded:
    """[rows + 64, width] (or [rows + 64]) on the device: the live rows hold `src` or NaN, the guard rows the sentinel"""

    def __init__(self, gpu, rows, width=None, src=None, offset=0):
        shape = (rows + GUARD_ROWS,) if width is None else (rows + GUARD_ROWS, width)
        numel = math.prod(shape)
        self.flat = torch.full((numel + offset,), SENTINEL, dtype=torch.float32, device=gpu)     # offset: floats off the allocation
        self.full = self.flat[offset:].view(shape)
        self.live = self.full[:rows]
        if src is None:
            self.live.fill_(float("nan"))
        else:
            self.live.copy_(src.to(gpu))

    @property
    def ptr(self):
        return C.c_void_p(self.full.data_ptr())

    def intact(self):
        bits = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32).item()
        guard = self.full[self.live.shape[0]:]
        head = self.flat[:self.flat.numel() - self.full.numel()]
        return bool((guard.contiguous().view(torch.int32) == bits).all()) and bool((head.view(torch.int32) == bits).all())


class Scratch:
    def __init__(self, gpu, nbytes):
        assert nbytes % 4 == 0
        self.words = nbytes // 4
        self.buf = torch.full((self.words + SCRATCH_GUARD // 4,), float("nan"), dtype=torch.float32, device=gpu)
        self.buf[self.words:] = SENTINEL
        self.nbytes = nbytes

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr())

    def intact(self):
        bits = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32).item()
        return bool((self.buf[self.words:].view(torch.int32) == bits).all())


def _lens(lengths):
    return (C.c_int64 * max(len(lengths), 1))(*lengths), len(lengths)


def _finish(tag, outputs, everything):
    """after the call: all guards intact, all live outputs finite; -> {name: live clone}"""
    torch.cuda.synchronize()
    for name, b in everything.items():
        assert b.intact(), "%s: guard of %s overwritten" % (tag, name)
    res = {}
    for name, b in outputs.items():
        assert bool(torch.isfinite(b.live).all()), "%s: %s has %d non-finite elements (a missed store?)" % (
            tag, name, int((~torch.isfinite(b.live)).sum()))
        res[name] = b.live.clone()
    return res


def spatial_raw(gpu, lengths, inputs, tag, use_att=True, use_xn=True, qk_offset=0, v_offset=0, expect=0):
    """ws_sphere_attention_fwd + _bwd on guarded, poisoned buffers; -> {att, xn, lse, dq, dk, dv}"""
    L = _lib()
    lib = L.lib()
    q, k, v, g_att, g_xn = inputs
    n, dq, dv = q.shape[0], q.shape[1], v.shape[1]
    lens, ns = _lens(lengths)
    st = L.current_stream()
    ins = {"q": Guarded(gpu, n, dq, q, qk_offset), "k": Guarded(gpu, n, dq, k, qk_offset), "v": Guarded(gpu, n, dv, v, v_offset),
           "g_att": Guarded(gpu, n, dv, g_att), "g_xn": Guarded(gpu, n, dv, g_xn)}
    fwd = {"att": Guarded(gpu, n, dv), "xn": Guarded(gpu, n, dv), "lse": Guarded(gpu, n)}
    rc = lib.ws_sphere_attention_fwd(ins["q"].ptr, ins["k"].ptr, ins["v"].ptr, n, dq, dv, lens, ns, fwd["att"].ptr, fwd["xn"].ptr,
                                     fwd["lse"].ptr, st)
    if expect:
        assert rc == expect, (tag, rc, lib.ws_last_error())
        fwd["att"].live.zero_()
        fwd["lse"].live.zero_()
    else:
        L.check(rc)
    res = {} if expect else _finish(tag + " forward", fwd, {**ins, **fwd})
    nbytes = lib.ws_sphere_attention_bwd_scratch_bytes(n, dv)
    assert nbytes >= (n * dv + n) * 4
    scratch = Scratch(gpu, nbytes)
    bwd = {"dq": Guarded(gpu, n, dq), "dk": Guarded(gpu, n, dq), "dv": Guarded(gpu, n, dv)}
    rc = lib.ws_sphere_attention_bwd(ins["q"].ptr, ins["k"].ptr, ins["v"].ptr, fwd["att"].ptr, fwd["lse"].ptr,
                                     ins["g_att"].ptr if use_att else None, ins["g_xn"].ptr if use_xn else None, n, dq, dv, lens, ns,
                                     bwd["dq"].ptr, bwd["dk"].ptr, bwd["dv"].ptr, scratch.ptr, scratch.nbytes, st)
    if expect:
        assert rc == expect, (tag, rc, lib.ws_last_error())
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(b.live).all()) for b in bwd.values()), "%s: a refused call wrote" % tag
        return None
    L.check(rc)
    res.update(_finish(tag + " backward", bwd, {**ins, **fwd, **bwd, "scratch": scratch}))
    return res


def channel_raw(gpu, lengths, inputs, max_minus, tag):
    """ws_channel_attention_fwd + _bwd on guarded, poisoned buffers; -> {a, out, dx1, dx2, dvalue}"""
    L = _lib()
    lib = L.lib()
    x1, x2, val, g_out = inputs
    n, c = x1.shape
    lens, ns = _lens(lengths)
    st = L.current_stream()
    ins = {"x1": Guarded(gpu, n, c, x1), "x2": Guarded(gpu, n, c, x2), "value": Guarded(gpu, n, c, val), "g_out": Guarded(gpu, n, c, g_out)}
    fwd = {"a": Guarded(gpu, ns * c, c), "out": Guarded(gpu, n, c)}
    scratch = Scratch(gpu, lib.ws_channel_attention_scratch_bytes(lens, ns, c, 0))
    L.check(lib.ws_channel_attention_fwd(ins["x1"].ptr, ins["x2"].ptr, ins["value"].ptr, n, c, lens, ns, int(max_minus), fwd["a"].ptr,
                                         fwd["out"].ptr, scratch.ptr, scratch.nbytes, st))
    res = _finish(tag + " forward", fwd, {**ins, **fwd, "scratch": scratch})
    scratch = Scratch(gpu, lib.ws_channel_attention_scratch_bytes(lens, ns, c, 1))
    bwd = {"dx1": Guarded(gpu, n, c), "dx2": Guarded(gpu, n, c), "dvalue": Guarded(gpu, n, c)}
    L.check(lib.ws_channel_attention_bwd(ins["x1"].ptr, ins["x2"].ptr, ins["value"].ptr, fwd["a"].ptr, ins["g_out"].ptr, n, c, lens, ns,
                                         int(max_minus), bwd["dx1"].ptr, bwd["dx2"].ptr, bwd["dvalue"].ptr, scratch.ptr, scratch.nbytes, st))
    res.update(_finish(tag + " backward", bwd, {**ins, **fwd, **bwd, "scratch": scratch}))
    return res


def _check(tag, got, r64, err32):
    for key, ref in r64.items():
        err = float((got[key].double().cpu() - ref).abs().max())
        print("branch %-30s %-6s kernel %.3e  float32 loop %.3e  ratio %.3f  max|ref| %.3e" % (
            tag, key, err, err32[key], err / err32[key], float(ref.abs().max())))
    bad = R.violations(got, r64, err32)
    assert not bad, (tag, bad)


def _same(a, b, tag, keys=None):
    for key in keys or a:
        assert torch.equal(a[key], b[key]), "%s: %s differs in %d elements" % (tag, key, int((a[key] != b[key]).sum()))


@pytest.mark.parametrize("row_id", [r["id"] for r in R.SPATIAL_ROWS])
def test_sphere_attention_branch(gpu, row_id):
    row = R.SPATIAL_BY_ID[row_id]
    inputs, r64, err32, _ = R.spatial_case(row_id)
    lengths = R.LENGTH_SETS[row["set"]]
    first = spatial_raw(gpu, lengths, inputs, row_id)
    _check(row_id, first, r64, err32)
    _same(first, spatial_raw(gpu, lengths, inputs, row_id + " again"), row_id + " run to run")


@pytest.mark.parametrize("row_id", [r["id"] for r in R.CHANNEL_ROWS])
def test_channel_attention_branch(gpu, row_id):
    row = R.CHANNEL_BY_ID[row_id]
    inputs, r64, err32, _ = R.channel_case(row_id)
    lengths = R.LENGTH_SETS[row["set"]]
    if row["kind"] == "elevation":
        assert float(inputs[0].abs().max()) > 100.0
    first = channel_raw(gpu, lengths, inputs, row["max_minus"], row_id)
    _check(row_id, first, r64, err32)
    _same(first, channel_raw(gpu, lengths, inputs, row["max_minus"], row_id + " again"), row_id + " run to run")


NULL_HALF_ROWS = ["dq8-dv192-edges-mild", "dq24-dv128-edges-mild", "dq40-dv320-edges-peaked"]      # one per NST


@pytest.mark.parametrize("row_id", NULL_HALF_ROWS)
def test_null_gradient_halves(gpu, row_id):
    """d_att == NULL and d_xn == NULL (reachable through the C entry alone: autograd hands zeros to backward) against the
    missing half as a zero tensor"""
    assert {R.SPATIAL_BY_ID[r]["nst"] for r in NULL_HALF_ROWS} == {2, 8, 16}
    q, k, v, g_att, g_xn = R.spatial_case(row_id)[0]
    lengths = R.LENGTH_SETS[R.SPATIAL_BY_ID[row_id]["set"]]
    zeros = torch.zeros_like(g_att)
    grads = ("dq", "dk", "dv")
    _same(spatial_raw(gpu, lengths, (q, k, v, g_att, g_xn), row_id + " d_att NULL", use_att=False),
          spatial_raw(gpu, lengths, (q, k, v, zeros, g_xn), row_id + " d_att zero"), row_id + " d_att NULL against zeros", grads)
    _same(spatial_raw(gpu, lengths, (q, k, v, g_att, g_xn), row_id + " d_xn NULL", use_xn=False),
          spatial_raw(gpu, lengths, (q, k, v, g_att, zeros), row_id + " d_xn zero"), row_id + " d_xn NULL against zeros", grads)


def test_alignment(gpu):
    """q and k one float off 16-byte alignment: same bits; v one float off: status 1 from both entries, nothing written"""
    row_id = "dq24-dv128-edges-mild"
    inputs = R.spatial_case(row_id)[0]
    lengths = R.LENGTH_SETS["edges"]
    aligned = spatial_raw(gpu, lengths, inputs, row_id)
    shifted = spatial_raw(gpu, lengths, inputs, row_id + " q, k + 4 bytes", qk_offset=1)
    _same(aligned, shifted, "q, k one float off")
    assert spatial_raw(gpu, lengths, inputs, row_id + " v + 4 bytes", v_offset=1, expect=1) is None
    assert b"aligned" in _lib().lib().ws_last_error()


def _ops_spatial(gpu, lengths, inputs):
    from weasal_amd import ops
    q, k, v, g_att, g_xn = (t.to(gpu) for t in inputs)
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    att, xn = ops.sphere_attention(q, k, v, lengths)
    torch.autograd.backward((att, xn), (g_att, g_xn))
    return {"att": att.detach(), "xn": xn.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}


def _ops_channel(gpu, lengths, inputs, max_minus):
    from weasal_amd import ops
    x1, x2, val, g_out = (t.to(gpu) for t in inputs)
    x1, x2, val = (t.requires_grad_(True) for t in (x1, x2, val))
    out = ops.channel_attention(x1, x2, val, lengths, max_minus)
    out.backward(g_out)
    return {"out": out.detach(), "dx1": x1.grad, "dx2": x2.grad, "dvalue": val.grad}


OPS_SPATIAL_ROWS = ["dq32-dv192-edges-peaked", "dq40-dv320-empties-ramp", "dq24-dv128-cap-ramp", "dq56-dv448-tall-ramp"]
OPS_CHANNEL_ROWS = ["channel-c100-mm1-edges", "channel-c96-mm1-empties", "channel-c64-mm0-cap"]


def test_ops_path_gives_the_bits_of_the_raw_calls(gpu):
    assert {R.SPATIAL_BY_ID[r]["set"] for r in OPS_SPATIAL_ROWS} == set(R.LENGTH_SETS)
    assert {R.CHANNEL_BY_ID[r]["set"] for r in OPS_CHANNEL_ROWS} == {r["set"] for r in R.CHANNEL_ROWS}
    for row_id in OPS_SPATIAL_ROWS:
        lengths = R.LENGTH_SETS[R.SPATIAL_BY_ID[row_id]["set"]]
        inputs = R.spatial_case(row_id)[0]
        _same(_ops_spatial(gpu, lengths, inputs), spatial_raw(gpu, lengths, inputs, row_id), row_id + " ops against raw")
    for row_id in OPS_CHANNEL_ROWS:
        row = R.CHANNEL_BY_ID[row_id]
        lengths = R.LENGTH_SETS[row["set"]]
        inputs = R.channel_case(row_id)[0]
        _same(_ops_channel(gpu, lengths, inputs, row["max_minus"]), channel_raw(gpu, lengths, inputs, row["max_minus"], row_id),
              row_id + " ops against raw")


def test_zero_rows_launch_nothing(gpu):
    """sphere form with lengths [0, 0, 0] and N = 0, channel form with no sphere: status 0, no launch, no store"""
    L = _lib()
    lib = L.lib()
    counter = C.c_longlong.in_dll(lib, "ws_launch_counter")
    st = L.current_stream()
    lens, ns = _lens([0, 0, 0])
    dq, dv, c = 24, 192, 36
    b = {name: Guarded(gpu, 0, w) for name, w in (("q", dq), ("k", dq), ("v", dv), ("att", dv), ("xn", dv), ("g", dv), ("dq", dq), ("dk", dq),
                                                 ("dv", dv), ("x", c), ("a", c), ("out", c))}
    b["lse"] = Guarded(gpu, 0)
    scratch = Scratch(gpu, 1024)
    torch.cuda.synchronize()
    before = counter.value
    assert lib.ws_sphere_attention_fwd(b["q"].ptr, b["k"].ptr, b["v"].ptr, 0, dq, dv, lens, ns, b["att"].ptr, b["xn"].ptr, b["lse"].ptr, st) == 0
    assert lib.ws_sphere_attention_bwd(b["q"].ptr, b["k"].ptr, b["v"].ptr, b["att"].ptr, b["lse"].ptr, b["g"].ptr, b["g"].ptr, 0, dq, dv,
                                       lens, ns, b["dq"].ptr, b["dk"].ptr, b["dv"].ptr, scratch.ptr, scratch.nbytes, st) == 0
    none, _ = _lens([])
    assert lib.ws_channel_attention_fwd(b["x"].ptr, b["x"].ptr, b["x"].ptr, 0, c, none, 0, 1, b["a"].ptr, b["out"].ptr, scratch.ptr,
                                        scratch.nbytes, st) == 0
    assert lib.ws_channel_attention_bwd(b["x"].ptr, b["x"].ptr, b["x"].ptr, b["a"].ptr, b["x"].ptr, 0, c, none, 0, 1, b["out"].ptr,
                                        b["out"].ptr, b["out"].ptr, scratch.ptr, scratch.nbytes, st) == 0
    assert counter.value == before
    torch.cuda.synchronize()
    assert all(g.intact() for g in b.values()) and scratch.intact() and bool(torch.isnan(scratch.buf[:scratch.words]).all())
