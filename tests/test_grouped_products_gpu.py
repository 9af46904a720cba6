"""GPU: the grouped dense-product launches (ws_priv_gemm_xb_group / ws_priv_gemm_xty_group, weasal_amd/csrc/gemm.hip;
grouped kernels and their launchers in gemm_xb.hip / gemm_xty.hip).

A grouped launch puts several mutually independent products of one kernel instantiation behind one grid and their
reductions behind one more; every member keeps the plan it gets alone.  So for every case here
  * each member's output is BIT-identical (torch.equal over the whole guarded buffer) to the same problem launched alone
    through today's entries,
  * it meets oracle/gemm_branch_ref.py's float64 reference within that module's per-element bound (the chain lengths read
    from the single launch's reporter string, as tests/test_gemm_branches_gpu.py does),
  * the buffers follow that test's conventions: NaN in the live region, a sentinel in the guard columns and the guard row,
    which must come back unchanged,
  * the number of launches (ws_launch_count) is the one the grouping rules give.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import priv_abi
from oracle import gemm_branch_ref as R
from weasal_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 12345.0
SLOPE = 0.1
DROP_P = 0.3
SEED = 0x1234567
BIG_PITCH = 1 << 23
V = C.c_void_p
XbProblem = priv_abi.struct("ws_xb_problem")          # laid out as weasal_amd/csrc/ws_common.h declares them
XtyProblem = priv_abi.struct("ws_xty_problem")


def _bind():
    for name in ("ws_priv_gemm_xb_group", "ws_priv_gemm_xty_group", "ws_priv_gemm_xb_ex", "ws_priv_gemm_xty_pitched"):
        priv_abi.entry(name)
    return _lib.lib()


def _p(t):
    return None if t is None else t.data_ptr()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(rows, n, ld, col0=0):
    y = torch.full((rows + 1, ld), SENT, dtype=torch.float32, device=DEV)
    y[:rows, col0:col0 + n] = float("nan")
    return y


def _launches(lib, fn):
    c0 = lib.ws_launch_count()
    fn()
    return lib.ws_launch_count() - c0


# ------------------------------------------------------------------------------------------------------------------
# xb members
# ------------------------------------------------------------------------------------------------------------------
class Xb:
    """one product with its operands on the device; epi: '' | 'bias' | 'res' | 'rrows' | 'gy' | 'mask' | 'drop' ('+'-joined)"""

    def __init__(self, seed, m, k, n, b="rows", epi="", act=False, scratch=False):
        lib = _lib.lib()
        rng = np.random.default_rng(seed)
        self.m, self.k, self.n, self.act = m, k, n, act
        e = set(epi.split("+")) if epi else set()
        self.x = (rng.standard_normal((m, k)) * np.exp(rng.normal(0.0, 1.0, size=(m, 1)))).astype(np.float32)
        self.bl = (rng.standard_normal((k, n)) / np.sqrt(k)).astype(np.float32)
        self.bias = rng.standard_normal(n).astype(np.float32) if "bias" in e else None
        self.rn = max(m // 2, 1) if "rrows" in e else m
        self.res = rng.standard_normal((max(self.rn, 1), n)).astype(np.float32) if ("res" in e or "rrows" in e) else None
        self.rld = 3 if "rrows" in e else 1
        self.rrows = None
        if "rrows" in e:
            idx = rng.integers(0, self.rn, size=m)
            idx[::7] = -1
            idx[3::11] = self.rn + 5
            self.rrows = np.full((max(m, 1) * self.rld,), 999999, np.int64)
            self.rrows[::self.rld][:m] = idx
        self.gy = None
        if "gy" in e:
            self.gy = rng.standard_normal((m, n)).astype(np.float32)
            self.gy.reshape(-1)[rng.integers(0, max(self.gy.size, 1), size=min(self.gy.size, 32))] = 0.0
        self.mask = ((rng.random((m, n)) < 0.7) * rng.integers(1, 256, size=(m, n))).astype(np.uint8) if "mask" in e else None
        self.mscale = float(np.float32(1.0) / np.float32(0.7))
        self.drop = "drop" in e
        self.ldx, self.ldy = k + 4, n + 8
        base = torch.zeros(max(m, 1) * self.ldx + 8, dtype=torch.float32, device=DEV)
        self.xd = base.as_strided((m, k), (self.ldx, 1))
        self.xd.copy_(torch.from_numpy(self.x))
        self._xbase = base
        if b == "t":                                              # row-major [n, ldw] read in place as its transpose
            ldw = k + 4
            bm = np.zeros((n, ldw), np.float32)
            bm[:, :k] = self.bl.T
            self.brs, self.bcs = 1, ldw
        else:
            bm = self.bl
            self.brs, self.bcs = -1, 1
        self.bd = _dev(bm)
        self.biasd, self.resd, self.rrd, self.gyd, self.mkd = _dev(self.bias), _dev(self.res), _dev(self.rrows), _dev(self.gy), _dev(self.mask)
        self.sb = max(int(lib.ws_gemm_xb_scratch_bytes(m, k, n)), 16) if scratch else 0
        self.scr = [torch.empty(self.sb, dtype=torch.uint8, device=DEV) if self.sb else None for _ in range(2)]

    def problem(self, ybuf, which):
        q = XbProblem()
        q.x, q.m, q.k, q.ldx = self.xd.data_ptr(), self.m, self.k, self.ldx
        q.b, q.b_row_stride, q.b_col_stride, q.n = self.bd.data_ptr(), self.brs, self.bcs, self.n
        q.bias, q.residual, q.ldr = _p(self.biasd), _p(self.resd), self.n
        q.res_rows, q.res_rows_ld, q.res_nrows = _p(self.rrd), self.rld, self.rn
        q.act, q.slope = 1 if self.act else 0, SLOPE
        q.gate_y, q.ldg, q.gate_slope = _p(self.gyd), self.n, SLOPE
        q.mask, q.ldm, q.mask_scale = _p(self.mkd), self.n, self.mscale
        q.drop_p, q.drop_seed = (DROP_P if self.drop else 0.0), SEED
        q.y, q.ldy = ybuf.data_ptr(), self.ldy
        q.scratch, q.scratch_bytes = _p(self.scr[which]), self.sb
        return q

    def alone(self, lib, ybuf):
        """today's single entries"""
        st = _lib.current_stream()
        common = (V(self.xd.data_ptr()), self.m, self.k, self.ldx, V(self.bd.data_ptr()), self.brs, self.bcs, self.n)
        act = 1 if self.act else 0
        if self.gy is not None or self.mask is not None:
            assert not self.drop and self.rrows is None
            return lib.ws_gemm_xb_gated_strided(*common, V(_p(self.biasd)), V(_p(self.resd)), self.n, act, SLOPE, V(_p(self.gyd)), self.n,
                                                SLOPE, V(_p(self.mkd)), self.n, self.mscale, V(ybuf.data_ptr()), self.ldy,
                                                V(_p(self.scr[0])), self.sb, st)
        return lib.ws_priv_gemm_xb_ex(*common, V(_p(self.biasd)), V(_p(self.resd)), self.n, V(_p(self.rrd)), self.rld, self.rn, act, SLOPE,
                                      DROP_P if self.drop else 0.0, SEED, V(ybuf.data_ptr()), self.ldy, V(_p(self.scr[0])), self.sb, st)

    def report(self, lib, ybuf):
        buf = C.create_string_buffer(256)
        _lib.check(lib.ws_gemm_xb_variant(V(self.xd.data_ptr()), self.m, self.k, self.ldx, V(self.bd.data_ptr()), self.brs, self.bcs, self.n,
                                          V(_p(self.biasd)), V(_p(self.resd)), self.n, V(_p(self.gyd)), self.n, V(_p(self.mkd)), self.n,
                                          V(ybuf.data_ptr()), self.ldy, V(_p(self.scr[1])), self.sb, buf, 256))
        return buf.value.decode()

    def check_oracle(self, got, plan, what):
        if self.m == 0:
            return
        resg = R.gathered(self.res, self.m, self.rrows, self.rld, self.rn) if self.res is not None else None
        gates = dict(act=self.act, slope=SLOPE, drop=(DROP_P, SEED, self.n) if self.drop else None, gate_y=self.gy, gate_slope=SLOPE,
                     mask=self.mask, mscale=self.mscale)
        ref = R.xb_ref(self.x, self.bl, self.bias, resg, **gates)
        splits, csplit = 1, None
        if "splits=" in plan:
            splits = int(plan.split("splits=")[1].split()[0])
            csplit = int(plan.split("csplit=")[1].split()[0])
        tol = R.xb_bound(self.x, self.bl, R.xb_chain(self.k, splits, csplit), self.bias, resg, **gates)
        msg = R.describe(got, ref, tol, what)
        assert not msg, msg


def run_xb_group(members, launches, plans=None):
    lib = _bind()
    ys = [_guarded(a.m, a.n, a.ldy) for a in members]            # launched alone
    yg = [_guarded(a.m, a.n, a.ldy) for a in members]            # grouped
    for a, y in zip(members, ys):
        _lib.check(a.alone(lib, y))
    arr = (XbProblem * len(members))(*[a.problem(y, 1) for a, y in zip(members, yg)])
    got = _launches(lib, lambda: _lib.check(lib.ws_priv_gemm_xb_group(arr, len(members), _lib.current_stream())))
    torch.cuda.synchronize()
    assert got == launches, "launches: %d, expected %d" % (got, launches)
    for i, (a, y1, y2) in enumerate(zip(members, ys, yg)):
        h1, h2 = y1.cpu().numpy(), y2.cpu().numpy()
        assert np.array_equal(h1.view(np.uint32), h2.view(np.uint32)), "member %d: grouped and single launches differ" % i
        live = h2[:a.m, :a.n].copy()
        h2[:a.m, :a.n] = SENT
        assert (h2.view(np.uint32) == np.float32(SENT).view(np.uint32)).all(), "member %d: a guard column / row changed" % i
        assert not np.isnan(live).any(), "member %d: an output element was not written" % i
        plan = a.report(lib, y2)
        if plans is not None and plans[i] is not None:
            assert plans[i] in plan, (i, plan)
        a.check_oracle(live, plan, "xb member %d" % i)


def test_xb_members_of_different_sizes_share_one_launch():
    """different m (ragged: 127, 33), k and n, all gemm_xb2_kernel<2, 2>; bias + LeakyReLU, residual + gate.y, gathered residual"""
    run_xb_group([Xb(1, 300, 64, 128, epi="bias", act=True), Xb(2, 127, 96, 160, epi="res+gy"), Xb(3, 33, 32, 256, epi="rrows+bias")], 1,
                 ["<NT=2, WN=2>"] * 3)


def test_xb_split_members_next_to_an_unsplit_one():
    """split-K members (full scratch) and an unsplit one: one product launch, one grouped split epilogue (mask, dropout bits)"""
    run_xb_group([Xb(4, 300, 1024, 128, epi="mask+bias", scratch=True), Xb(5, 300, 128, 128, epi="bias", act=True),
                  Xb(6, 127, 512, 128, epi="drop+res", act=True, scratch=True)], 2,
                 ["<NT=2, WN=2> b=rows epilogue=staged splits=4 csplit=8 + splitk_epilogue_kernel", "splits=1 csplit=4",
                  "splits=2 csplit=8 + splitk_epilogue_kernel"])


def test_xb_one_split_member_keeps_the_single_epilogue():
    """(a single splitk_epilogue_kernel launch counts with its product, as in the single entry: one)"""
    run_xb_group([Xb(7, 300, 1024, 128, scratch=True), Xb(8, 300, 128, 128)], 1, ["splits=4 csplit=8", "splits=1"])


def test_xb_transposed_b_next_to_row_major():
    run_xb_group([Xb(9, 200, 64, 128, b="t", epi="bias"), Xb(10, 200, 64, 128, epi="gy")], 1, ["b=transposed", "b=rows"])


def test_xb_empty_member_and_other_instantiations():
    """m == 0 does nothing (the buffer keeps its guard row); <NT=1, WN=2> (n = 48) and the generic kernel (k = 40) fall out of
    the <2, 2> group and run alone"""
    run_xb_group([Xb(11, 300, 64, 128, epi="bias"), Xb(12, 0, 64, 128), Xb(13, 300, 64, 48, epi="res"), Xb(14, 90, 40, 128, epi="bias", act=True),
                  Xb(15, 64, 64, 128, epi="mask")], 3,
                 ["<NT=2, WN=2>", "none (m == 0)", "<NT=1, WN=2>", "gemm_xb_kernel<NT=2", "<NT=2, WN=2>"])


@pytest.mark.parametrize("count,launches", [(1, 1), (9, 2), (19, 3)])
def test_xb_counts(count, launches):
    """one member is the single launch; nine members of one instantiation spill into a second launch (8 + 1); a list longer
    than one call plans at once (16) is taken in slices: 8 + 8, then one of 3"""
    run_xb_group([Xb(20 + i, 40 + 13 * i, 32 * (1 + i % 3), 128, epi=("bias", "res", "gy")[i % 3], act=i % 2 == 0) for i in range(count)],
                 launches)


# ------------------------------------------------------------------------------------------------------------------
# xty members
# ------------------------------------------------------------------------------------------------------------------
_BIG = {}


class Xty:
    def __init__(self, seed, m, k, n, ldo=0, col0=0, out=None, big=False):
        lib = _lib.lib()
        rng = np.random.default_rng(seed)
        self.m, self.k, self.n, self.ldo, self.col0 = m, k, n, ldo, col0
        self.x = (rng.standard_normal((m, k)) * np.exp(rng.normal(0.0, 1.0, size=(m, 1)))).astype(np.float32)
        self.y = rng.standard_normal((m, n)).astype(np.float32)
        self.ldx = BIG_PITCH if big else k + 2
        self.ldy = n + 2
        if big:                                                   # chunk (64) * pitch * 4 >= 2^31: the 32-bit-overflow form
            if "t" not in _BIG:
                _BIG["t"] = torch.empty(33 * BIG_PITCH + 64, dtype=torch.float32, device=DEV)
            xb = _BIG["t"]
        else:
            xb = torch.zeros(max(m, 1) * self.ldx + 8, dtype=torch.float32, device=DEV)
        self.xd = xb.as_strided((m, k), (self.ldx, 1))
        self.xd.copy_(torch.from_numpy(self.x))
        yb = torch.zeros(max(m, 1) * self.ldy + 8, dtype=torch.float32, device=DEV)
        self.yd = yb.as_strided((m, n), (self.ldy, 1))
        self.yd.copy_(torch.from_numpy(self.y))
        self._keep = (xb, yb)
        self.sb = max(int(lib.ws_gemm_xty_scratch_bytes(m, k, n)), 16)
        self.scr = [torch.empty(self.sb, dtype=torch.uint8, device=DEV) for _ in range(2)]

    def out_buffer(self):
        if self.ldo:
            return _guarded(self.k, self.n, self.ldo, self.col0)
        o = torch.full((self.k * self.n + 64,), SENT, dtype=torch.float32, device=DEV)
        o[:self.k * self.n] = float("nan")
        return o

    def out_ptr(self, obuf):
        return obuf.data_ptr() + 4 * self.col0

    def problem(self, obuf, which):
        q = XtyProblem()
        q.x, q.m, q.k, q.ldx = self.xd.data_ptr(), self.m, self.k, self.ldx
        q.y, q.n, q.ldy = self.yd.data_ptr(), self.n, self.ldy
        q.out, q.ldo = self.out_ptr(obuf), self.ldo
        q.scratch, q.scratch_bytes = self.scr[which].data_ptr(), self.sb
        return q

    def alone(self, lib, obuf):
        st = _lib.current_stream()
        a = (V(self.xd.data_ptr()), self.m, self.k, self.ldx, V(self.yd.data_ptr()), self.n, self.ldy, V(self.out_ptr(obuf)))
        if self.ldo:
            return lib.ws_priv_gemm_xty_pitched(*a, self.ldo, V(self.scr[0].data_ptr()), st)
        return lib.ws_gemm_xty(*a, V(self.scr[0].data_ptr()), st)

    def report(self, lib, obuf):
        buf = C.create_string_buffer(256)
        _lib.check(lib.ws_gemm_xty_variant(V(self.xd.data_ptr()), self.m, self.k, self.ldx, V(self.yd.data_ptr()), self.n, self.ldy,
                                           V(self.out_ptr(obuf)), self.ldo, V(self.scr[1].data_ptr()), 0, buf, 256))
        return buf.value.decode()

    def live(self, h):
        if self.ldo:
            got = h[:self.k, self.col0:self.col0 + self.n].copy()
            h[:self.k, self.col0:self.col0 + self.n] = SENT
        else:
            got = h[:self.k * self.n].reshape(self.k, self.n).copy()
            h[:self.k * self.n] = SENT
        return got


def run_xty_group(members, launches, plans, shared=None):
    """shared: {member index: index of the member whose output buffer it writes a column block of}"""
    lib = _bind()
    shared = shared or {}
    bufs = []
    for which in range(2):
        row = []
        for i, a in enumerate(members):
            row.append(row[shared[i]] if i in shared else a.out_buffer())
            if i in shared:
                row[i][:a.k, a.col0:a.col0 + a.n] = float("nan")
        bufs.append(row)
    for a, o in zip(members, bufs[0]):
        _lib.check(a.alone(lib, o))
    arr = (XtyProblem * len(members))(*[a.problem(o, 1) for a, o in zip(members, bufs[1])])
    got = _launches(lib, lambda: _lib.check(lib.ws_priv_gemm_xty_group(arr, len(members), _lib.current_stream())))
    torch.cuda.synchronize()
    assert got == launches, "launches: %d, expected %d" % (got, launches)
    for i, a in enumerate(members):
        assert torch.equal(bufs[0][i].view(torch.int32), bufs[1][i].view(torch.int32)), "member %d: grouped and single launches differ" % i
    hosts = {}
    for i, a in enumerate(members):
        key = shared.get(i, i)
        if key not in hosts:
            hosts[key] = bufs[1][key].cpu().numpy()
        live = a.live(hosts[key])
        plan = a.report(lib, bufs[1][i])
        assert plans[i] in plan, (i, plan)
        if a.m == 0:
            assert (live == 0).all(), "member %d: an empty product must clear its output" % i
            continue
        assert not np.isnan(live).any(), "member %d: an output element was not written" % i
        chunk = int(plan.split("chunk=")[1].split()[0])
        chunks = int(plan.split("chunks=")[1].split()[0])
        msg = R.describe(live, R.xty_ref(a.x, a.y), R.xty_bound(a.x, a.y, chunk, chunks), "xty member %d" % i)
        assert not msg, msg
    for key, h in hosts.items():
        assert (h.view(np.uint32) == np.float32(SENT).view(np.uint32)).all(), "buffer %d: an element outside dW changed" % key


def test_xty_wide_and_grouped_reductions_and_a_single_chunk():
    """gemm_xty2_kernel<2, 2, 2, 2> three times: chunks > 1 with the wide reduction (65 536 elements), chunks > 1 with the
    32-element form, one chunk written flat without a reduction: one product launch, one grouped reduction"""
    run_xty_group([Xty(31, 2000, 256, 256), Xty(32, 1500, 128, 128), Xty(33, 20, 128, 128)], 2,
                  ["WN=2, TI=float> chunk=128 chunks=16 reduce=reduce_partials_wide_kernel out=flat", "reduce=reduce_partials_kernel out=flat",
                   "chunks=1 reduce=none out=flat"])


def test_xty_two_column_blocks_of_one_matrix():
    """the two halves of a decoder step's dW [128, 192 + 128] as pitched members writing one buffer"""
    run_xty_group([Xty(34, 300, 128, 128, ldo=320, col0=192), Xty(35, 77, 128, 192, ldo=320, col0=0)], 2,
                  ["out=pitched", "out=pitched"], shared={1: 0})


def test_xty_empty_member_other_instantiation_and_the_overflow_form():
    """m == 0 clears its output (flat and pitched); <1, 1, 1, 1> (k = n = 32) shares nobody's instantiation and launches its
    product alone but its chunk sums ride in the grouped reduction; the 32-bit-overflow form (gemm_xty_kernel, row pitch
    2^23) runs alone, reduction and all"""
    run_xty_group([Xty(36, 900, 128, 128), Xty(37, 0, 64, 96), Xty(38, 0, 32, 64, ldo=72, col0=4), Xty(39, 700, 32, 32), Xty(40, 640, 160, 128),
                   Xty(41, 33, 32, 32, big=True)], 4,
                  ["KT=2, NT=2, WK=2, WN=2", "memset (m == 0) out=flat", "memset (m == 0) out=pitched", "KT=1, NT=1, WK=1, WN=1",
                   "KT=2, NT=2, WK=2, WN=2", "gemm_xty_kernel<NT=1, KT=1>"])


@pytest.mark.parametrize("count,launches", [(1, 2), (9, 4), (18, 6)])
def test_xty_counts(count, launches):
    """one member: its product and its reduction; nine: products 8 + 1, reductions 8 + 1; eighteen (slices of 16): products and
    reductions 8 + 8, then 1 + 1 for the slice of two"""
    run_xty_group([Xty(50 + i, 400 + 37 * i, 128, 128) for i in range(count)], launches, ["KT=2, NT=2, WK=2, WN=2"] * count)


def test_xty_member_scratch_is_checked():
    lib = _bind()
    a = Xty(60, 1500, 128, 128)
    q = a.problem(a.out_buffer(), 1)
    q.scratch_bytes = a.sb - 256
    arr = (XtyProblem * 1)(q)
    assert lib.ws_priv_gemm_xty_group(arr, 1, _lib.current_stream()) == 5 and b"scratch too small" in lib.ws_last_error()
