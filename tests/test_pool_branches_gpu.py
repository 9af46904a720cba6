"""Every launch branch of the pooling kernels (weasal_amd/csrc/pools.hip) and of the transposed table (csr.hip, scan.hip)
against the exact references of oracle/pool_ref.py.

Data.  Every max-pool case runs on three data sets:
  * "mixed": x small integers in [-3, 3] (ties everywhere, ties with the zero shadow row, duplicate supports in a row), dy and
    add integers in [-2, 2]: every sum is exact in f32 and a bf16 store rounds an exact integer once, so out, arg and dx
    must EQUAL the reference whatever the order of the sums;
  * "negative": x in [-3, -1]: shadow columns win, the padded columns of the unrolled neighbour loop must not;
  * "normal": randn: the forward is bit-equal, the backward is held per element to (n + 8) 2^-24 sum|terms| (bf16: times
    (1 + 2^-8), + 2^-8 |ref|), n and sum|terms| from the reference.  Never a fraction of the tensor's maximum.
Index matrices always hold shadow entries, a support nobody points at, a crowded support, and supports with list lengths
1 ... 9 (as far as the pairs go): the ladder of the backward's 4-pair unroll.

Orders.  None (the plain entries), a random permutation and the identity (the _ordered entries): out, arg and dx must be
bit-identical under all three, on normal data too -- the pair lists are sorted, so the sums run in the same order.  Every
backward runs twice and must repeat its bits.

The case tables below are plain data.  Which form a call takes is the library's own statement: ws_pool_variant formats the
plan functions the launchers dispatch on (pools.hip: max_pool_plan, closest_fwd_plan, closest_bwd_plan).  Every launch made
here asks it first, with the device pointers of the run, and must get a name of case_plans();
tests/test_pool_branches_cpu.py asserts that those names are every form the plan functions produce.
"""
import contextlib
import ctypes as C
import functools
import zlib

import numpy as np
import pytest
import torch

import priv_abi
from oracle import pool_ref as P
from weasal_amd import _lib, ops
from weasal_amd._lib import check, current_stream, ptr

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
ORDERS = (None, "perm", "identity")
DATA = ("mixed", "negative", "normal")


def _g(op, c):
    """lanes per row of the vectorised max-pool kernels: the case tables need it at import time, before the library is
    loaded; tests/test_pool_branches_cpu.py holds it to the reporter's G= for every width of MAX_ROWS"""
    if op == "fwd" and c <= 16:
        return 4
    return 8 if c <= 32 else 16 if c <= 64 else 32 if c <= 128 else 64


def small_sizes(c):
    """(nq, ns, h) around the rows-per-wave S = 64 / G of the forward (nq) and of the backward (ns): one row, S - 1, S,
    S + 1 (a partial last group), 7 S (fewer than 8 groups: an empty eighth), 8 S + 3; h below, at and off the unroll
    widths 4 and 8.  The (8 S + 3, 21) size carries the whole list-length ladder."""
    sf, sb = 64 // _g("fwd", c), 64 // _g("bwd", c)
    raw = [(1, 7 * sb, 9), (sf - 1, sb + 1, 3), (sf, sb, 4), (sf + 1, sb - 1, 5), (7 * sf, 1, 8),
           (8 * sf + 3, 8 * sb + 3, 21), (8 * sf + 3, 7 * sb, 1)]
    out = []
    for nq, ns, h in raw:
        out.append((max(nq, 1), max(ns, 1), h))              # (S = 1: the S - 1 sizes are one row again, at another h)
    return out


def _row(c, dtype, note, sizes=None, shift=0, orders=ORDERS):
    return dict(id="c%d_%s%s%s" % (c, dtype, "_shift" if shift else "", "" if sizes is None else "_n%d" % sizes[0][0]),
                c=c, dtype=dtype, shift=shift, sizes=sizes or small_sizes(c), orders=orders, note=note)


MAX_ROWS = []
for _c, _note in ((4, "G=4 forward; G=8 backward with idle lanes"), (16, "G=4 forward; G=8 backward"), (20, "G=8, idle lanes"),
                  (32, "G=8"), (36, "G=16, idle lanes"), (64, "G=16"), (68, "G=32, idle lanes"), (128, "G=32"),
                  (132, "G=64, one partial trip"), (256, "G=64, one trip"), (260, "split 2, a 4-channel last chunk"),
                  (512, "split 2"), (1024, "split 4"), (5, "generic kernel"), (30, "generic kernel")):
    for _d in ("f32", "bf16"):
        MAX_ROWS.append(_row(_c, _d, _note))
MAX_ROWS += [
    _row(64, "f32", "generic kernel on a vectorisable width: rows 4 bytes off 16-byte alignment", shift=1),
    _row(64, "bf16", "generic kernel on a vectorisable width: rows 2 bytes off 8-byte alignment", shift=1),
    # 8200 rows: no channel split, every wave walks its row's chunks; 8200 groups: several interleaved trips per wave
    _row(260, "f32", "unsplit G=64, two trips (the second partial); > 8192 groups", sizes=[(8200, 8200, 3)]),
    _row(512, "f32", "unsplit G=64, two trips; > 8192 groups", sizes=[(8200, 8200, 3)]),
    # more groups than 4 waves x 4096 workgroups: ws_block_range hands out chunks longer than 4 groups
    _row(132, "f32", "un-ordered past the grid cap: contiguous multi-item chunks", sizes=[(16400, 16400, 2)], orders=(None,)),
]

# (c, nq, ns, h) of the byte-record forms (ws_priv_max_pool_fwd_u8 / _bwd_u8): what the fused strided blocks run
U8_CASES = [(16, 37, 29, 5), (32, 37, 29, 9), (64, 37, 29, 21), (128, 37, 29, 3), (128, 37, 29, 8), (128, 37, 29, 9),
            (128, 37, 29, 59), (256, 23, 19, 4), (512, 23, 19, 5), (1024, 11, 9, 3),
            (64, 64, 300, 255), (128, 61, 300, 255)]           # h = 255: the largest the record holds (255 % 4, 255 % 8 != 0)

CLOSEST_FWD = [(c, d, h) for c in (1, 5, 64, 130) for d in ("f32", "bf16") for h in (1, 4)]
# (c, dtype, shift, h): h = 1 is the column-0 table ops.closest_pool builds, h = 4 the full table (pairs of other columns skipped)
CLOSEST_BWD = [(c, "f32", 0, h) for c in (32, 64, 128, 256, 512) for h in (1, 4)] + \
              [(20, "f32", 0, 1), (96, "f32", 0, 4), (64, "bf16", 0, 1), (64, "f32", 1, 4)]

TABLE_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 2047, 2048, 2049, 3001)
TABLE_NS = (0, 1, 4093, 4094, 4095, 4096, 8191)              # the scan runs over ns + 2 slots: one tile up to 4094
TABLE_NS_3LEVEL = 16777215                                    # 4097 tiles: the smallest three-level scan


# ------------------------------------------------------------------------------------------------------------------
# the library's own statement of a launch: ws_pool_variant
# ------------------------------------------------------------------------------------------------------------------
POOL_OPS = dict(max_fwd=0, max_bwd=1, closest_fwd=2, closest_bwd=3)      # WS_POOL_* (include/weasal_hip.h)
FAKE_ARG = 0x30000000


def variant(op, dtype, c, rows, rows_a, rows_b, arg=None, arg_bytes=4, ordered=False):
    """(name, grid) of the launch an entry makes; rows = nq (forwards) or ns (backwards); rows_a / rows_b / arg are
    addresses (only their alignment counts)"""
    buf, grid = C.create_string_buffer(128), C.c_int32(-1)
    check(_lib.lib().ws_pool_variant(POOL_OPS[op], rows, c, rows_a, rows_b, arg, int(dtype == "bf16"), arg_bytes, int(ordered),
                                     buf, 128, C.byref(grid)))
    return buf.value.decode(), grid.value


def fake_rows(dtype, shift=0):
    """the two row addresses the GPU run sees, alignment-wise: allocations are 256-byte aligned, `shift` elements into one"""
    off = shift * (2 if dtype == "bf16" else 4)
    return 0x10000000 + off, 0x20000000 + off


@contextlib.contextmanager
def closest_vec_switch(value):
    """ws_closest_bwd_vec set to `value`, put back afterwards"""
    flag = C.c_int.in_dll(_lib.lib(), "ws_closest_bwd_vec")
    keep = flag.value
    flag.value = value
    try:
        yield
    finally:
        flag.value = keep


@functools.lru_cache(None)
def case_plans():
    """the ws_pool_variant name of every launch the tables above make"""
    plans = set()
    for r in MAX_ROWS:
        a, b = fake_rows(r["dtype"], r["shift"])
        for nq, ns, _h in r["sizes"]:
            for o in r["orders"]:
                plans.add(variant("max_fwd", r["dtype"], r["c"], nq, a, b, FAKE_ARG, ordered=o is not None)[0])
                plans.add(variant("max_bwd", r["dtype"], r["c"], ns, a, b, FAKE_ARG, ordered=o is not None)[0])
    a, b = fake_rows("f32")
    for c, nq, ns, _h in U8_CASES:
        for o in (False, True):
            plans.add(variant("max_fwd", "f32", c, nq, a, b, FAKE_ARG, 1, o)[0])
            plans.add(variant("max_bwd", "f32", c, ns, a, b, FAKE_ARG, 1, o)[0])
    for c, d, _h in CLOSEST_FWD:
        plans.add(variant("closest_fwd", d, c, 1, *fake_rows(d))[0])
    for c, d, shift, _h in CLOSEST_BWD:
        for flag in (1, 0):
            with closest_vec_switch(flag):
                plans.add(variant("closest_bwd", d, c, 1, *fake_rows(d, shift))[0])
    return frozenset(plans)


def reported(op, rows, c, a, b, arg=None, arg_bytes=4, order=None):
    """before a launch: the reporter answers for its device pointers (status 0) with a name the case tables are known by"""
    name, grid = variant(op, "bf16" if a.dtype == torch.bfloat16 else "f32", c, rows, ptr(a), ptr(b), ptr(arg), arg_bytes,
                         order is not None)
    assert name in case_plans() and grid >= 1, (name, grid)


# ------------------------------------------------------------------------------------------------------------------
# data
# ------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def make_inds(rng, nq, h, ns):
    """[nq, h] int64 with values in [0, ns]: shadow entries (= ns) in the even rows only, one support nobody points at, one
    crowded support, supports with exactly 1 ... 9 pairs (as far as nq * h and ns go), the rest spread over the other supports"""
    n = nq * h
    perm = rng.permutation(ns)
    crowd = perm[1] if ns >= 2 else perm[0]                   # (perm[0] stays empty when there are 3 supports or more)
    ladder = perm[2:12] if ns >= 3 else perm[:0]
    others = perm[12:] if ns > 12 else np.array([crowd])
    even = np.arange(n).reshape(nq, h)[0::2].reshape(-1)     # the shadow entries sit in the even rows: odd rows have none,
    n_sh = min(max(1, n // 6), even.size) if n >= 2 else 0    # so with all-negative x only padded columns could lift them
    vals = [ns] * n_sh
    for k, s in enumerate(ladder[:9]):
        if len(vals) + k + 1 <= n // 2 + 1:
            vals += [s] * (k + 1)
    vals += [crowd] * min(n // 4 + 1, 150, n - len(vals))  # (capped: a very long list costs the table's slow sort branch)
    rest = n - len(vals)
    real = np.concatenate([np.asarray(vals[n_sh:], np.int64), others[rng.integers(0, others.size, size=rest)]])
    flat = np.full(n, ns, np.int64)
    sh_at = rng.permutation(even)[:n_sh]
    flat[np.setdiff1d(np.arange(n), sh_at)] = rng.permutation(real)
    return flat.reshape(nq, h)


def make_rows(rng, data, shape, dtype, what):
    """numpy f32 rows of a data set, already representable in `dtype`; what: "x" or "g" (dy, add)"""
    if data == "normal":
        a = rng.standard_normal(shape).astype(np.float32)
        return torch.from_numpy(a).to(DT[dtype]).float().numpy()
    if what == "g":
        return rng.integers(-2, 3, size=shape).astype(np.float32)
    lo, hi = (-3, 0) if data == "negative" else (-3, 4)
    return rng.integers(lo, hi, size=shape).astype(np.float32)


def dev(a, dtype, gpu, shift=0):
    """device copy of numpy `a` as torch `dtype`, its first element `shift` elements past an aligned allocation"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.empty(t.numel() + shift, dtype=dtype, device=gpu)
    v = buf[shift:].view(t.shape)
    v.copy_(t)
    return v


def blank(shape, dtype, gpu, shift=0):
    """an output buffer full of a value no kernel writes (NaN, -7 for integers): an element left out shows"""
    n = int(np.prod(shape))
    fill = float("nan") if dtype.is_floating_point else (249 if dtype == torch.uint8 else -7)
    buf = torch.full((n + shift,), fill, dtype=dtype, device=gpu)
    return buf[shift:].view(shape)


def make_order(kind, n, rng, gpu):
    if kind is None:
        return None
    o = rng.permutation(n) if kind == "perm" else np.arange(n)
    return torch.from_numpy(o.astype(np.int32)).to(gpu)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------
# launches through the C ABI
# ------------------------------------------------------------------------------------------------------------------
def max_fwd(x, inds, order, shift=0):
    lib = _lib.lib()
    (ns, c), (nq, h) = x.shape, inds.shape
    out = blank((nq, c), x.dtype, x.device, shift)
    arg = blank((nq, c), torch.int32, x.device)
    sfx = "_bf16" if x.dtype == torch.bfloat16 else ""
    reported("max_fwd", nq, c, x, out, arg, order=order)
    if order is None:
        check(getattr(lib, "ws_max_pool_fwd" + sfx)(ptr(x), ns, c, ptr(inds), nq, h, ptr(out), ptr(arg), current_stream()))
    else:
        check(getattr(lib, "ws_max_pool_fwd_ordered" + sfx)(ptr(x), ns, c, ptr(inds), nq, h, ptr(out), ptr(arg), ptr(order),
                                                          current_stream()))
    return out, arg


def max_bwd(dy, arg, table, order, shift=0):
    lib = _lib.lib()
    nq, c = dy.shape
    dx = blank((table.ns, c), dy.dtype, dy.device, shift)
    sfx = "_bf16" if dy.dtype == torch.bfloat16 else ""
    reported("max_bwd", table.ns, c, dy, dx, arg, order=order)
    if order is None:
        check(getattr(lib, "ws_max_pool_bwd" + sfx)(ptr(dy), ptr(arg), nq, table.h, c, ptr(table.offsets), ptr(table.pairs),
                                                  table.ns, ptr(dx), current_stream()))
    else:
        check(getattr(lib, "ws_max_pool_bwd_ordered" + sfx)(ptr(dy), ptr(arg), nq, table.h, c, ptr(table.offsets),
                                                          ptr(table.pairs), table.ns, ptr(dx), ptr(order), current_stream()))
    return dx


def u8_entries():
    """the byte-record forms: exported by the library, declared in csrc/ws_common.h (not in include/weasal_hip.h)"""
    return priv_abi.entry("ws_priv_max_pool_fwd_u8"), priv_abi.entry("ws_priv_max_pool_bwd_u8")


def closest_fwd(x, inds):
    lib = _lib.lib()
    (ns, c), (nq, h) = x.shape, inds.shape
    out = blank((nq, c), x.dtype, x.device)
    name = "ws_closest_pool_fwd" + ("_bf16" if x.dtype == torch.bfloat16 else "")
    reported("closest_fwd", nq, c, x, out)
    check(getattr(lib, name)(ptr(x), ns, c, ptr(inds), nq, h, ptr(out), current_stream()))
    return out


def closest_bwd(dy, table, shift=0):
    lib = _lib.lib()
    nq, c = dy.shape
    dx = blank((table.ns, c), dy.dtype, dy.device, shift)
    name = "ws_closest_pool_bwd" + ("_bf16" if dy.dtype == torch.bfloat16 else "")
    reported("closest_bwd", table.ns, c, dy, dx)
    check(getattr(lib, name)(ptr(dy), nq, table.h, c, ptr(table.offsets), ptr(table.pairs), table.ns, ptr(dx), current_stream()))
    return dx


def assert_bound(dx, ref, n, sabs, bf16, what):
    msg = P.describe(f64(dx), ref, P.bwd_bound(n, sabs, ref, bf16), what)
    assert not msg, msg


def rounded(ref, dtype):
    """an exact float64 integer result as the kernel stores it: one rounding to `dtype`"""
    return torch.from_numpy(ref).to(torch.float32).to(dtype)


# ------------------------------------------------------------------------------------------------------------------
# max-pool
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", MAX_ROWS, ids=[r["id"] for r in MAX_ROWS])
def test_max_pool_branch(gpu, row):
    c, dtype, shift = row["c"], DT[row["dtype"]], row["shift"]
    bf = dtype == torch.bfloat16
    for nq, ns, h in row["sizes"]:
        rng = _rng(row["id"], nq, ns, h)
        inds_np = make_inds(rng, nq, h, ns)
        assert (inds_np == ns).any() or nq * h < 2
        inds = torch.from_numpy(inds_np).to(gpu)
        table = ops.TransposedTable(inds, ns)
        orders_q = [make_order(k, nq, rng, gpu) for k in row["orders"]]
        orders_s = [make_order(k, ns, rng, gpu) for k in row["orders"]]
        for data in DATA:
            what = "%s nq=%d ns=%d h=%d %s" % (row["id"], nq, ns, h, data)
            x_np = make_rows(rng, data, (ns, c), row["dtype"], "x")
            dy_np = make_rows(rng, data, (nq, c), row["dtype"], "g")
            ref_out, ref_arg = P.max_pool_ref(x_np, inds_np)
            ref_dx, n, sabs = P.max_pool_bwd_ref(dy_np, ref_arg, inds_np, ns)
            x, dy = dev(x_np, dtype, gpu, shift), dev(dy_np, dtype, gpu, shift)
            want_out, want_arg = torch.from_numpy(ref_out).to(gpu), torch.from_numpy(ref_arg).to(gpu)
            first = None
            for oq, osup, kind in zip(orders_q, orders_s, row["orders"]):
                out, arg = max_fwd(x, inds, oq, shift)
                assert torch.equal(out.float(), want_out), "%s order=%s: out" % (what, kind)
                assert torch.equal(arg, want_arg), "%s order=%s: arg (the first maximum wins)" % (what, kind)
                dx = max_bwd(dy, arg, table, osup, shift)
                again = max_bwd(dy, arg, table, osup, shift)
                assert torch.equal(bits(dx), bits(again)), "%s order=%s: the backward does not repeat its bits" % (what, kind)
                if data == "normal":
                    assert_bound(dx, ref_dx, n, sabs, bf, "%s order=%s: dx" % (what, kind))
                else:
                    assert torch.equal(dx.cpu(), rounded(ref_dx, dtype)), "%s order=%s: dx" % (what, kind)
                if first is None:
                    first = (out, arg, dx)
                else:
                    for a, b, name in zip(first, (out, arg, dx), ("out", "arg", "dx")):
                        assert torch.equal(bits(a), bits(b)), "%s: %s depends on the order (%s)" % (what, name, kind)
            if data == "normal" and (nq, ns, h) == row["sizes"][-1] and not shift:
                # the same case through the operator: the _ordered entries with no order registered, autograd's backward
                ops.clear_batch_hints()
                xg = x.clone().requires_grad_(True)
                y = ops.max_pool(xg, inds)
                assert torch.equal(bits(y.detach()), bits(first[0])), "%s: ops.max_pool" % what
                gx, = torch.autograd.grad(y, xg, dy)
                assert torch.equal(bits(gx), bits(first[2])), "%s: ops.max_pool backward" % what
                ops.clear_batch_hints()


# ------------------------------------------------------------------------------------------------------------------
# the byte arg-max record
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", U8_CASES, ids=["c%d_nq%d_h%d" % (c, nq, h) for c, nq, _, h in U8_CASES])
def test_max_pool_byte_record(gpu, case):
    c, nq, ns, h = case
    fwd8, bwd8 = u8_entries()
    rng = _rng("u8", case)
    inds_np = make_inds(rng, nq, h, ns)
    inds = torch.from_numpy(inds_np).to(gpu)
    table = ops.TransposedTable(inds, ns)
    for data in DATA:
        what = "u8 c=%d nq=%d ns=%d h=%d %s" % (c, nq, ns, h, data)
        x_np = make_rows(rng, data, (ns, c), "f32", "x")
        dy_np = make_rows(rng, data, (nq, c), "f32", "g")
        add_np = make_rows(rng, data, (ns, c), "f32", "g")
        ref_out, ref_arg = P.max_pool_ref(x_np, inds_np)
        x, dy, add = dev(x_np, torch.float32, gpu), dev(dy_np, torch.float32, gpu), dev(add_np, torch.float32, gpu)
        pub_out, pub_arg = max_fwd(x, inds, None)
        assert torch.equal(pub_arg.cpu(), torch.from_numpy(ref_arg)), what
        pub_dx = max_bwd(dy, pub_arg, table, None)
        for okind in (None, "perm"):
            oq, osup = make_order(okind, nq, rng, gpu), make_order(okind, ns, rng, gpu)
            out = blank((nq, c), torch.float32, gpu)
            arg8 = blank((nq, c), torch.uint8, gpu)
            reported("max_fwd", nq, c, x, out, arg8, 1, oq)
            check(fwd8(ptr(x), ns, c, ptr(inds), nq, h, ptr(out), ptr(arg8), ptr(oq), current_stream()))
            assert torch.equal(out.cpu(), torch.from_numpy(ref_out)), "%s order=%s: out" % (what, okind)
            assert torch.equal(arg8.to(torch.int32), pub_arg), "%s order=%s: the byte record differs from the int32 one" % (what, okind)
            for a_np, a in ((None, None), (add_np, add)):
                dx = blank((ns, c), torch.float32, gpu)
                reported("max_bwd", ns, c, dy, dx, arg8, 1, osup)
                check(bwd8(ptr(dy), ptr(arg8), nq, h, c, ptr(table.offsets), ptr(table.pairs), ns, ptr(dx), ptr(osup), ptr(a),
                           current_stream()))
                tag = "%s order=%s add=%s: dx" % (what, okind, a is not None)
                # the kernel's association: the pool sum first, then + add -- one f32 addition on top of the public result
                assert torch.equal(bits(dx), bits(pub_dx if a is None else pub_dx + a)), tag + " against the public backward"
                ref_dx, n, sabs = P.max_pool_bwd_ref(dy_np, ref_arg, inds_np, ns, a_np)
                if data == "normal":
                    assert_bound(dx, ref_dx, n, sabs, False, tag)
                else:
                    assert torch.equal(dx.cpu(), rounded(ref_dx, torch.float32)), tag


# ------------------------------------------------------------------------------------------------------------------
# closest-pool
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,dtype,h", CLOSEST_FWD, ids=["c%d_%s_h%d" % t for t in CLOSEST_FWD])
def test_closest_pool_forward(gpu, c, dtype, h):
    nq, ns = 71, 23
    rng = _rng("cf", c, dtype, h)
    inds_np = make_inds(rng, nq, h, ns)
    inds_np[:3, 0] = ns                                       # shadow in column 0: zero rows
    inds = torch.from_numpy(inds_np).to(gpu)
    for data in ("mixed", "normal"):
        x_np = make_rows(rng, data, (ns, c), dtype, "x")
        out = closest_fwd(dev(x_np, DT[dtype], gpu), inds)
        assert torch.equal(out.float().cpu(), torch.from_numpy(P.closest_pool_ref(x_np, inds_np))), (c, dtype, h, data)


def closest_ladder_inds(rng, c, h):
    """column 0 gives support k exactly k pairs, k = 0 ... 2 S + 1 for the vector form's S = 64 / G rows side by side (two
    trips of S unrolled: every remainder of the slot loop), then a crowded support, an empty one, shadow entries"""
    s_par = max(1, 64 // min(c // 4, 64)) if c >= 4 else 1
    top = 2 * s_par + 1
    col0 = np.concatenate([np.full(k, k) for k in range(top + 1)] + [np.full(3 * top + 7, top + 1), np.full(5, top + 3)])
    ns = top + 3                                              # support top + 2 stays empty; top + 3 == ns: shadow
    col0 = rng.permutation(col0)
    inds = rng.integers(0, ns + 1, size=(col0.size, h)).astype(np.int64)
    inds[:, 0] = col0
    return inds, ns


@pytest.mark.parametrize("c,dtype,shift,h", CLOSEST_BWD, ids=["c%d_%s_s%d_h%d" % t for t in CLOSEST_BWD])
def test_closest_pool_backward(gpu, c, dtype, shift, h):
    rng = _rng("cb", c, dtype, shift, h)
    inds_np, ns = closest_ladder_inds(rng, c, h)
    nq = inds_np.shape[0]
    inds = torch.from_numpy(inds_np).to(gpu)
    table = ops.TransposedTable(inds, ns)
    for data in ("mixed", "normal"):
        dy_np = make_rows(rng, data, (nq, c), dtype, "g")
        ref, n, sabs = P.closest_pool_bwd_ref(dy_np, inds_np, ns)
        assert n[:, 0].max() > n[:-3, 0].max() and (n[:, 0] == 0).sum() >= 2
        dy = dev(dy_np, DT[dtype], gpu, shift)
        got = {}
        for f in (1, 0):
            with closest_vec_switch(f):
                got[f] = closest_bwd(dy, table, shift)
                what = "closest bwd c=%d %s shift=%d h=%d %s vec=%d" % (c, dtype, shift, h, data, f)
                assert torch.equal(bits(got[f]), bits(closest_bwd(dy, table, shift))), what + ": does not repeat its bits"
            if data == "normal":
                assert_bound(got[f], ref, n, sabs, dtype == "bf16", what)
            else:
                assert torch.equal(got[f].cpu(), rounded(ref, DT[dtype])), what
        if data == "mixed":
            assert torch.equal(bits(got[1]), bits(got[0]))


# ------------------------------------------------------------------------------------------------------------------
# transposed table and scan
# ------------------------------------------------------------------------------------------------------------------
def check_table(table, inds_np, ns):
    off_ref, pairs_ref = P.transposed_table_ref(inds_np, ns)
    off = table.offsets.cpu().numpy().astype(np.int64)
    assert off.shape == (ns + 2,)
    assert np.array_equal(off, off_ref), "offsets: first difference at slot %d" % int(np.argmax(off != off_ref))
    assert off[ns + 1] == off[ns] == pairs_ref.size           # shadow pairs are not tabulated: slot ns stays empty
    pairs = table.pairs.cpu().numpy().astype(np.int64)[:pairs_ref.size]
    if not np.array_equal(pairs, pairs_ref):
        p = int(np.argmax(pairs != pairs_ref))
        s = int(np.searchsorted(off_ref, p, side="right")) - 1
        raise AssertionError("list of support %d (length %d): element %d is %d, not %d"
                             % (s, off_ref[s + 1] - off_ref[s], p - off_ref[s], pairs[p], pairs_ref[p]))


def test_table_sort_branches(gpu):
    """list lengths at the edges of the three sort branches of tr_sort_lists: counting rank (<= 64), LDS bitonic (65 ... 2048,
    padded to a power of two), odd-even in global memory (> 2048); the pair order is what makes every backward deterministic"""
    rng = _rng("sort")
    ns, nq, h = len(TABLE_LENGTHS), 800, 16
    flat = np.full(nq * h, ns, np.int64)
    flat[:sum(TABLE_LENGTHS)] = np.repeat(np.arange(ns), TABLE_LENGTHS)
    inds_np = rng.permutation(flat).reshape(nq, h)
    table = ops.TransposedTable(torch.from_numpy(inds_np).to(gpu), ns)
    off = table.offsets.cpu().numpy()
    assert tuple(np.diff(off[:ns + 1])) == TABLE_LENGTHS
    check_table(table, inds_np, ns)


@pytest.mark.parametrize("ns", TABLE_NS)
def test_table_scan_tiles(gpu, ns):
    """ns around the one-tile / two-level boundary of ws_exclusive_scan_i32 (ns + 2 slots, 4096 per tile)"""
    rng = _rng("scan", ns)
    nq, h = 500, 6
    inds_np = rng.integers(0, ns + 1, size=(nq, h)).astype(np.int64)
    if ns >= 2:
        inds_np[0, :2] = (0, ns - 1)                          # the first and the last support
        inds_np[1, :3] = ns
    check_table(ops.TransposedTable(torch.from_numpy(inds_np).to(gpu), ns), inds_np, ns)


def test_table_scan_three_levels(gpu):
    """ns = 2^24 - 1: 4097 tiles, so the tile sums themselves need two levels (the scratch arithmetic of
    ws_scan_scratch_items matters for the first time).  Compared on the device, in int64, slab by slab."""
    ns = TABLE_NS_3LEVEL
    rng = _rng("scan3")
    nq, h = 1000, 5
    inds_np = rng.integers(0, ns, size=(nq, h)).astype(np.int64)
    inds_np[rng.random((nq, h)) < 0.1] = ns
    inds_np[0, :3] = (0, ns - 1, ns - 1)
    inds_np[7, :2] = (4095, 4096)
    inds_np[8, :2] = (4096 * 4096 - 2, 4096 * 4096 - 1)       # around the first slot of the 4097th tile
    inds = torch.from_numpy(inds_np).to(gpu)
    table = ops.TransposedTable(inds, ns)
    flat = inds.reshape(-1)
    live = flat[flat < ns]
    carry = torch.zeros((), dtype=torch.int64, device=gpu)
    slab = 1 << 21
    for lo in range(0, ns + 1, slab):
        hi = min(lo + slab, ns + 1)                            # slots lo ... hi - 1 of offsets[0 ... ns]
        cnt = torch.bincount(live[(live >= lo) & (live < hi)] - lo, minlength=hi - lo)
        want = carry + torch.cumsum(cnt, 0) - cnt              # exclusive, int64
        got = table.offsets[lo:hi].to(torch.int64)
        bad = got != want
        assert not bool(bad.any()), "offsets: first difference at slot %d" % (lo + int(bad.nonzero()[0]))
        carry = carry + cnt.sum()
    assert int(table.offsets[ns]) == int(table.offsets[ns + 1]) == int(live.numel()) == int(carry)
    # the lists: ascending pair ids of every support that has any
    flat_np = inds_np.reshape(-1)
    ids = np.nonzero(flat_np < ns)[0]
    want_pairs = ids[np.argsort(flat_np[ids], kind="stable")]
    assert np.array_equal(table.pairs.cpu().numpy()[:want_pairs.size].astype(np.int64), want_pairs)
    sup = torch.from_numpy(np.unique(flat_np[ids])).to(gpu)
    beg = table.offsets[sup].cpu().numpy().astype(np.int64)
    assert np.array_equal(flat_np[want_pairs[beg]], sup.cpu().numpy())      # every list starts where offsets says


def test_table_degenerate(gpu):
    """nq = 0 (no pair at all) and an all-shadow matrix: every offset is 0"""
    for ns in (0, 5):
        t = ops.TransposedTable(torch.zeros((0, 3), dtype=torch.int64, device=gpu), ns)
        assert torch.equal(t.offsets.cpu(), torch.zeros(ns + 2, dtype=torch.int32))
        inds_np = np.full((9, 4), ns, np.int64)
        t = ops.TransposedTable(torch.from_numpy(inds_np).to(gpu), ns)
        check_table(t, inds_np, ns)
        assert not t.offsets.any()


# ------------------------------------------------------------------------------------------------------------------
# degenerate calls (C ABI)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", (5, 16, 512))
def test_degenerate_calls(gpu, c):
    lib = _lib.lib()
    st = current_stream()
    h = 3
    for dtype, sfx in ((torch.float32, ""), (torch.bfloat16, "_bf16")):
        x = torch.ones((4, c), dtype=dtype, device=gpu)
        none_i = torch.zeros((0, h), dtype=torch.int64, device=gpu)
        out0 = torch.empty((0, c), dtype=dtype, device=gpu)
        arg0 = torch.empty((0, c), dtype=torch.int32, device=gpu)
        t0 = ops.TransposedTable(none_i, 4)
        # nq = 0: the forwards do nothing, the backwards write zeros (no pair reaches a support)
        assert getattr(lib, "ws_max_pool_fwd" + sfx)(ptr(x), 4, c, ptr(none_i), 0, h, ptr(out0), ptr(arg0), st) == 0
        assert getattr(lib, "ws_closest_pool_fwd" + sfx)(ptr(x), 4, c, ptr(none_i), 0, h, ptr(out0), st) == 0
        dx = blank((4, c), dtype, gpu)
        assert getattr(lib, "ws_max_pool_bwd" + sfx)(ptr(out0), ptr(arg0), 0, h, c, ptr(t0.offsets), ptr(t0.pairs), 4, ptr(dx), st) == 0
        assert not dx.float().cpu().numpy().any()
        dx = blank((4, c), dtype, gpu)
        assert getattr(lib, "ws_closest_pool_bwd" + sfx)(ptr(out0), 0, h, c, ptr(t0.offsets), ptr(t0.pairs), 4, ptr(dx), st) == 0
        assert not dx.float().cpu().numpy().any()
        # ns = 0: every index is the shadow: the forward gives zeros and arg 0, the backwards have nothing to write
        nq = 7
        shadow = torch.zeros((nq, h), dtype=torch.int64, device=gpu)
        ts = ops.TransposedTable(shadow, 0)
        dy = torch.ones((nq, c), dtype=dtype, device=gpu)
        for order in (None, make_order("perm", nq, _rng("deg", c), gpu)):
            out = blank((nq, c), dtype, gpu)
            arg = blank((nq, c), torch.int32, gpu)
            if order is None:
                rc = getattr(lib, "ws_max_pool_fwd" + sfx)(None, 0, c, ptr(shadow), nq, h, ptr(out), ptr(arg), st)
            else:
                rc = getattr(lib, "ws_max_pool_fwd_ordered" + sfx)(None, 0, c, ptr(shadow), nq, h, ptr(out), ptr(arg), ptr(order), st)
            assert rc == 0
            assert not out.float().cpu().numpy().any() and not arg.cpu().numpy().any()
        out = blank((nq, c), dtype, gpu)
        assert getattr(lib, "ws_closest_pool_fwd" + sfx)(None, 0, c, ptr(shadow), nq, h, ptr(out), st) == 0
        assert not out.float().cpu().numpy().any()
        assert getattr(lib, "ws_max_pool_bwd" + sfx)(ptr(dy), ptr(arg), nq, h, c, ptr(ts.offsets), ptr(ts.pairs), 0, None, st) == 0
        assert getattr(lib, "ws_closest_pool_bwd" + sfx)(ptr(dy), nq, h, c, ptr(ts.offsets), ptr(ts.pairs), 0, None, st) == 0
    torch.cuda.synchronize()
