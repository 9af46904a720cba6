"""Tables and references of the attention launch-branch tests (test_attention_branches_cpu.py, test_attention_branches_gpu.py).

  * the launch rules of weasal_amd/csrc/attention.hip, restated in plain Python from its comments and launchers (not imported
    from the library: this is the independent statement the tables are checked against);
  * four sphere-length sets, three input regimes, SPATIAL_ROWS and CHANNEL_ROWS: every row carries the launch it claims to reach;
  * the inputs, the float64 reference (tests/att_ref.py) and the float32 yardstick of every row, computed once and shared;
  * the bound of the GPU test;
  * the two attention forms and their gradients written out by hand in float64 (`spatial_manual`, `channel_manual`): with
    `defect=None` they are att_ref, with `defect=1 .. 11` they differ from it by exactly one defect.  The CPU test shows that
    the bound rejects every one of them: the GPU test would notice a kernel that made that mistake.
"""
import functools

import torch

import att_ref

# ---- launch rules (attention.hip: launch_pv, launch_dqk, the chunk loop of sphere_att_dqk_kernel, att_spheres) ---------------
TILE = 64                       # rows per tile, own and streamed
MAX_SPHERES = 64


def nst_of(dq):
    """MFMA steps of 4 over dq: the instantiation the launchers pick"""
    return 2 if dq <= 8 else 8 if dq <= 32 else 16


def ct_of(dv):
    """16-column tiles of one dv slice of the forward / dV kernel"""
    return 8 if dv % 128 == 0 else 4


def slices_of(dv):
    return dv // (16 * ct_of(dv))


def ot_of(dq):
    """16-column output tiles of the dQ / dK kernel"""
    return (4 * nst_of(dq) + 15) // 16


def ot_mask(dq):
    """'full' (every output tile stored whole), 'partial' (a tile stored in part) and / or 'masked' (a tile not stored at all)"""
    out = set()
    for ot in range(ot_of(dq)):
        live = min(max(dq - 16 * ot, 0), 16)
        out.add("full" if live == 16 else "masked" if live == 0 else "partial")
    return out


def chunk_walk(dv):
    """the dv chunks sphere_att_dqk_kernel stages, in order"""
    return [128] * (dv // 128) + ([64] if dv % 128 else [])


def tiles_of(n):
    return (n + TILE - 1) // TILE


def spatial_launch(dq, dv):
    return (nst_of(dq), ct_of(dv), slices_of(dv), ot_of(dq), tuple(chunk_walk(dv)))


def channel_strided(c):
    """the backward reads A^T / dE^T through the product's strides (True) or from the transposed copies (False)"""
    return c % 32 == 0


def lane_elems(c):
    """softmax elements per lane: one wave per row, lane l holds columns l, l + 64, ..."""
    return (c + 63) // 64


def lane_class(c):
    if c < 64:
        return "1 idle"
    if c == 64:
        return "1"
    if c == 512:
        return "8"
    return "%d%s" % (lane_elems(c), "" if c % 64 == 0 else " partial")


# ---- sphere-length sets ------------------------------------------------------------------------------------------------
LENGTH_SETS = {
    "edges": [1, 63, 64, 0, 65, 130],
    "empties": [0, 0, 5, 0, 128, 0, 257, 0, 0],
    "cap": [(i * 37) % 71 for i in range(64)],
    "tall": [700],
}
ROWS_OF = {name: sum(v) for name, v in LENGTH_SETS.items()}
assert ROWS_OF == {"edges": 323, "empties": 390, "cap": 2172, "tall": 700}

REGIMES = ("mild", "ramp", "peaked")
AMPLITUDE = {"mild": 0.5, "ramp": 2.0, "peaked": 6.0, "large": 2.0}
TEETH_MAX_ROWS = 400            # the wrong references run on the rows with at most this many stacked rows


def _spatial_row(dq, dv, lset, regime):
    return {"id": "dq%d-dv%d-%s-%s" % (dq, dv, lset, regime), "dq": dq, "dv": dv, "set": lset, "regime": regime}


def _claim(row, nst, ct, slices, ot, walk):
    row.update(nst=nst, ct=ct, slices=slices, ot=ot, walk=tuple(walk))
    return row


# (dq, dv, length set, regime) and the claimed (NST, CT, slices, OT, chunk walk)
SPATIAL_ROWS = [
    # the 64-sphere cap: every (NST, CT)
    _claim(_spatial_row(8, 64, "cap", "ramp"), 2, 4, 1, 1, [64]),
    _claim(_spatial_row(8, 128, "cap", "peaked"), 2, 8, 1, 1, [128]),
    _claim(_spatial_row(16, 64, "cap", "mild"), 8, 4, 1, 2, [64]),
    _claim(_spatial_row(24, 128, "cap", "ramp"), 8, 8, 1, 2, [128]),
    _claim(_spatial_row(32, 256, "cap", "ramp"), 8, 8, 2, 2, [128, 128]),
    _claim(_spatial_row(48, 64, "cap", "peaked"), 16, 4, 1, 4, [64]),
    _claim(_spatial_row(64, 384, "cap", "mild"), 16, 8, 3, 4, [128, 128, 128]),
    # leading, trailing and consecutive empty spheres, two full tiles, five key tiles: every (NST, CT)
    _claim(_spatial_row(8, 192, "empties", "peaked"), 2, 4, 3, 1, [128, 64]),
    _claim(_spatial_row(8, 128, "empties", "ramp"), 2, 8, 1, 1, [128]),
    _claim(_spatial_row(32, 192, "empties", "ramp"), 8, 4, 3, 2, [128, 64]),
    _claim(_spatial_row(32, 256, "empties", "peaked"), 8, 8, 2, 2, [128, 128]),
    _claim(_spatial_row(40, 320, "empties", "ramp"), 16, 4, 5, 4, [128, 128, 64]),
    _claim(_spatial_row(64, 512, "empties", "peaked"), 16, 8, 4, 4, [128, 128, 128, 128]),
    # eleven query and key tiles: every NST
    _claim(_spatial_row(8, 64, "tall", "peaked"), 2, 4, 1, 1, [64]),
    _claim(_spatial_row(24, 128, "tall", "peaked"), 8, 8, 1, 2, [128]),
    _claim(_spatial_row(56, 448, "tall", "ramp"), 16, 4, 7, 4, [128, 128, 128, 64]),
    _claim(_spatial_row(64, 384, "tall", "peaked"), 16, 8, 3, 4, [128, 128, 128]),
    # the length set of test_attention_gpu.py at the widths it does not run
    _claim(_spatial_row(8, 128, "edges", "mild"), 2, 8, 1, 1, [128]),
    _claim(_spatial_row(8, 192, "edges", "mild"), 2, 4, 3, 1, [128, 64]),
    _claim(_spatial_row(16, 64, "edges", "peaked"), 8, 4, 1, 2, [64]),
    _claim(_spatial_row(24, 128, "edges", "mild"), 8, 8, 1, 2, [128]),
    _claim(_spatial_row(32, 192, "edges", "peaked"), 8, 4, 3, 2, [128, 64]),
    _claim(_spatial_row(40, 320, "edges", "peaked"), 16, 4, 5, 4, [128, 128, 64]),
    _claim(_spatial_row(48, 64, "edges", "ramp"), 16, 4, 1, 4, [64]),
    _claim(_spatial_row(56, 448, "edges", "mild"), 16, 4, 7, 4, [128, 128, 128, 64]),
    _claim(_spatial_row(64, 384, "edges", "ramp"), 16, 8, 3, 4, [128, 128, 128]),
    _claim(_spatial_row(64, 512, "edges", "mild"), 16, 8, 4, 4, [128, 128, 128, 128]),
]
SPATIAL_BY_ID = {r["id"]: r for r in SPATIAL_ROWS}


def _channel_row(c, max_minus, lset, strided, lanes, kind="channel"):
    return {"id": "%s-c%d-mm%d-%s" % (kind, c, int(max_minus), lset), "c": c, "max_minus": bool(max_minus), "set": lset,
            "kind": kind, "strided": strided, "lanes": lanes}


# (c, max_minus, length set) and the claimed (strided backward, softmax lane class)
CHANNEL_ROWS = [
    _channel_row(4, True, "edges", False, "1 idle"), _channel_row(4, False, "edges", False, "1 idle"),
    _channel_row(12, True, "edges", False, "1 idle"), _channel_row(12, False, "edges", False, "1 idle"),
    _channel_row(36, True, "edges", False, "1 idle"), _channel_row(36, False, "edges", False, "1 idle"),
    _channel_row(64, True, "edges", True, "1"), _channel_row(64, False, "edges", True, "1"),
    _channel_row(96, True, "edges", True, "2 partial"), _channel_row(96, False, "edges", True, "2 partial"),
    _channel_row(100, True, "edges", False, "2 partial"), _channel_row(100, False, "edges", False, "2 partial"),
    _channel_row(256, True, "edges", True, "4"), _channel_row(256, False, "edges", True, "4"),
    _channel_row(512, True, "edges", True, "8"), _channel_row(512, False, "edges", True, "8"),
    # 64 spheres: 64 forward and 192 backward products, in slices of 16 and groups of 8
    _channel_row(12, True, "cap", False, "1 idle"), _channel_row(64, False, "cap", True, "1"),
    _channel_row(100, True, "cap", False, "2 partial"),
    _channel_row(36, False, "empties", False, "1 idle"), _channel_row(96, True, "empties", True, "2 partial"),
    # ele_att's operands at tile heights (energies of 1e5 - 1e6, a one-hot softmax)
    _channel_row(96, False, "edges", True, "2 partial", kind="elevation"),
    # added for the dense-product reporter sweep (test_attention_branches_cpu.py): the two product forms the widths above miss
    _channel_row(32, True, "edges", True, "1 idle"),        # gemm_xb2_kernel<NT=1, WN=1>
    _channel_row(132, False, "edges", False, "3 partial"),  # gemm_xb_kernel<NT=4>
]
CHANNEL_BY_ID = {r["id"]: r for r in CHANNEL_ROWS}


# ---- inputs, float64 reference, float32 yardstick ----------------------------------------------------------------------------
def _ramp(x, lengths):
    out = x.clone()
    for a, b in att_ref.spans(lengths):
        if b > a:
            out[a:b] *= torch.linspace(0.1, 3.0, b - a).unsqueeze(1)
    return out


def _pair(regime, n, w, lengths, g):
    amp = AMPLITUDE[regime]
    a = (torch.rand((n, w), generator=g) * 2 - 1) * amp
    b = (torch.rand((n, w), generator=g) * 2 - 1) * amp
    return a, (_ramp(b, lengths) if regime == "ramp" else b)


def _errors(r32, r64):
    return {key: float((r32[key].double() - r64[key]).abs().max()) for key in r64}


@functools.lru_cache(maxsize=None)
def spatial_inputs(row_id):
    """(q, k, v, g_att, g_xn) of a row, float32 on the CPU"""
    row = SPATIAL_BY_ID[row_id]
    lengths = LENGTH_SETS[row["set"]]
    n, dq, dv = sum(lengths), row["dq"], row["dv"]
    g = torch.Generator().manual_seed(4000 + 7 * dq + dv + 1000 * REGIMES.index(row["regime"]) + 10000 * sorted(LENGTH_SETS).index(row["set"]))
    q, k = _pair(row["regime"], n, dq, lengths, g)
    v = torch.rand((n, dv), generator=g) * 2 - 1
    g_att, g_xn = torch.rand((n, dv), generator=g) * 2 - 1, torch.rand((n, dv), generator=g) * 2 - 1
    return q, k, v, g_att, g_xn


@functools.lru_cache(maxsize=None)
def spatial_case(row_id):
    """inputs, the float64 reference and the float32 loop's error against it (computed once, shared, never modified)"""
    inputs = spatial_inputs(row_id)
    lengths = LENGTH_SETS[SPATIAL_BY_ID[row_id]["set"]]
    r64 = att_ref.spatial_with_grads(*inputs[:3], lengths, *inputs[3:])
    r32 = att_ref.spatial_with_grads(*inputs[:3], lengths, *inputs[3:], dtype=torch.float32)
    return inputs, r64, _errors(r32, r64), r32


ELEVATION_CENTRES = (271.0, 288.5, 263.0, 255.0, 297.0, 280.0)


@functools.lru_cache(maxsize=None)
def channel_inputs(row_id):
    """(x1, x2, value, g_out) of a row, float32 on the CPU: regime `large` of test_attention_gpu.py, or ele_att's operands as
    the network forms them on a tile (heights with centre heights of 255 - 297 m through two 2 -> c projections)"""
    row = CHANNEL_BY_ID[row_id]
    lengths = LENGTH_SETS[row["set"]]
    n, c = sum(lengths), row["c"]
    g = torch.Generator().manual_seed(5000 + c + 7 * int(row["max_minus"]) + 10000 * sorted(LENGTH_SETS).index(row["set"]))
    if row["kind"] == "elevation":
        assert len(lengths) == len(ELEVATION_CENTRES)
        h = torch.rand((n, 1), generator=g) * 3 - 1.5
        centre = torch.cat([torch.full((b - a, 1), z) for (a, b), z in zip(att_ref.spans(lengths), ELEVATION_CENTRES)])
        ele = torch.cat((h, h + centre), dim=1)
        w1, w2 = ((torch.rand((2, c), generator=g) * 2 - 1) / 2 ** 0.5 for _ in range(2))
        x1, x2 = torch.nn.functional.leaky_relu(ele @ w1, 0.1), torch.nn.functional.leaky_relu(ele @ w2, 0.1)
    else:
        x1, x2 = _pair("large", n, c, lengths, g)
    val = torch.rand((n, c), generator=g) * 2 - 1
    g_out = torch.rand((n, c), generator=g) * 2 - 1
    return x1, x2, val, g_out


@functools.lru_cache(maxsize=None)
def channel_case(row_id):
    row = CHANNEL_BY_ID[row_id]
    inputs = channel_inputs(row_id)
    lengths = LENGTH_SETS[row["set"]]
    r64 = att_ref.channel_with_grads(*inputs[:3], lengths, row["max_minus"], inputs[3])
    r32 = att_ref.channel_with_grads(*inputs[:3], lengths, row["max_minus"], inputs[3], dtype=torch.float32)
    return inputs, r64, _errors(r32, r64), r32


# ---- the bound ---------------------------------------------------------------------------------------------------------
def bound(key, r64, err32):
    """max |kernel - ref64| <= 4 * max |att_ref in float32 on the CPU - ref64| + 1e-6 * max |ref64|   (test_attention_gpu.py)"""
    return 4.0 * err32[key] + 1e-6 * float(r64[key].abs().max())


def violations(got, r64, err32):
    """[(tensor, error, yardstick, bound)] of the tensors of `got` (anything indexable by the keys of r64) outside the bound;
    a non-finite error counts as outside"""
    bad = []
    for key, ref in r64.items():
        err = float((got[key].detach().double().cpu() - ref).abs().max())
        if not err <= bound(key, r64, err32):
            bad.append((key, err, err32[key], bound(key, r64, err32)))
    return bad


# ---- the two forms by hand, float64, with one defect each ------------------------------------------------------------------------
SPATIAL_DEFECTS = {
    1: "the last key of every sphere is masked out",
    2: "the last key tile of a sphere also takes the first row of the next sphere",
    3: "the accumulator is not rescaled at one key-tile boundary where the running maximum rises, though l is",
    4: "xn is divided by the previous sphere's n",
    5: "D = rowsum(dO o att) is formed without the d_xn / n term",
    6: "dK uses the log-sum-exp and D of the key row instead of the query row",
    7: "dQ and dK columns from 16 * (dq // 16) on are zero",
    8: "dO V^T leaves out the last 64 columns",
}
CHANNEL_DEFECTS = {
    9: "dVal uses A instead of A^T",
    10: "dE keeps the plain sign in the max-minus form",
    11: "softmax and its backward ignore columns from 64 * ((c - 1) // 64) on",
}


def defect_applies(defect, row):
    if defect == 3:
        return max(LENGTH_SETS[row["set"]]) > TILE          # (and the maximum has to rise: max_rises, asserted by the CPU test)
    if defect == 4:
        return len(LENGTH_SETS[row["set"]]) > 1
    if defect == 7:
        return row["dq"] % 16 != 0
    if defect == 8:
        return row["dv"] % 128 != 0
    if defect == 10:
        return row["max_minus"]
    if defect == 11:
        return row["c"] > 64
    return True


def _streamed(s, v, skip_rescale_once):
    """softmax(s) v the way the forward kernel forms it: key tiles of 64, running maximum m, running sum l, the accumulator
    rescaled by exp(m_old - m_new).  skip_rescale_once: leave the accumulator (not l) unscaled at the first tile boundary
    where some row's maximum rises.  -> (att, whether that boundary existed)"""
    n = s.shape[0]
    m = torch.full((n,), -float("inf"), dtype=s.dtype)
    l = torch.zeros((n,), dtype=s.dtype)
    acc = torch.zeros((n, v.shape[1]), dtype=s.dtype)
    skipped = False
    for k0 in range(0, s.shape[1], TILE):
        st = s[:, k0:k0 + TILE]
        mx = torch.maximum(m, st.max(dim=1)[0])
        sc = torch.exp(m - mx)
        p = torch.exp(st - mx[:, None])
        l = l * sc + p.sum(dim=1)
        if skip_rescale_once and not skipped and k0 > 0 and bool((mx > m).any()):
            skipped = True
        else:
            acc = acc * sc[:, None]
        acc = acc + p @ v[k0:k0 + TILE]
        m = mx
    return acc / l[:, None], skipped


def max_rises(q, k, lengths):
    """whether in some sphere some query row's running maximum rises at a key-tile boundary after the first tile"""
    q, k = q.double(), k.double()
    for a, b in att_ref.spans(lengths):
        if b - a > TILE:
            s = q[a:b] @ k[a:b].T
            run = s[:, :TILE].max(dim=1)[0]
            for k0 in range(TILE, b - a, TILE):
                nxt = s[:, k0:k0 + TILE].max(dim=1)[0]
                if bool((nxt > run).any()):
                    return True
                run = torch.maximum(run, nxt)
    return False


def spatial_manual(q, k, v, lengths, g_att, g_xn, defect=None):
    """{att, xn, dq, dk, dv} in float64 from the formulas of attention.hip's header; `defect`: a key of SPATIAL_DEFECTS"""
    q, k, v, g_att, g_xn = (t.detach().to("cpu", torch.float64) for t in (q, k, v, g_att, g_xn))
    total, dq_w = q.shape[0], q.shape[1]
    out = {key: torch.zeros_like(v) for key in ("att", "xn", "dv")}
    out.update(dq=torch.zeros_like(q), dk=torch.zeros_like(k))
    rescale_skipped = False
    prev_n = None
    for a, b in att_ref.spans(lengths):
        n = b - a
        if n == 0:
            prev_n = n
            continue
        ke, ve = k[a:b], v[a:b]
        if defect == 2 and b < total:
            ke, ve = k[a:b + 1], v[a:b + 1]
        s = q[a:b] @ ke.T
        if defect == 1 and n >= 2:
            s[:, n - 1] = -float("inf")
        lse = torch.logsumexp(s, dim=1)
        p = torch.exp(s - lse[:, None])
        if defect == 3 and not rescale_skipped:
            att, rescale_skipped = _streamed(s, ve, True)
        else:
            att = p @ ve
        n_xn = float(prev_n) if (defect == 4 and prev_n is not None) else float(n)
        xn = att / n_xn
        d_o = g_att[a:b] + g_xn[a:b] / float(n)
        dsum = ((g_att[a:b] if defect == 5 else d_o) * att).sum(dim=1)
        vb, ob = (ve[:, :-64], d_o[:, :-64]) if defect == 8 else (ve, d_o)
        dp = ob @ vb.T
        ds = p * (dp - dsum[:, None])
        d_q = ds @ ke
        if defect == 6:                                     # L and D by the key row (square part; the keys are the queries)
            lk, dk_ = lse[:n], dsum[:n]
            d_k = (torch.exp(s[:, :n] - lk[None, :]) * (dp[:, :n] - dk_[None, :])).T @ q[a:b]
        else:
            d_k = (ds.T @ q[a:b])[:n]
        d_v = (p.T @ d_o)[:n]
        if defect == 7:
            d_q[:, 16 * (dq_w // 16):] = 0.0
            d_k[:, 16 * (dq_w // 16):] = 0.0
        out["att"][a:b], out["xn"][a:b], out["dq"][a:b], out["dk"][a:b], out["dv"][a:b] = att, xn, d_q, d_k, d_v
        prev_n = n
    return out


def channel_manual(x1, x2, value, lengths, max_minus, g_out, defect=None):
    """{out, dx1, dx2, dvalue} in float64 from the formulas of attention.hip's header; `defect`: a key of CHANNEL_DEFECTS"""
    x1, x2, value, g_out = (t.detach().to("cpu", torch.float64) for t in (x1, x2, value, g_out))
    c = x1.shape[1]
    live = 64 * ((c - 1) // 64) if defect == 11 else c
    out = {key: torch.zeros_like(x1) for key in ("out", "dx1", "dx2", "dvalue")}
    for a, b in att_ref.spans(lengths):
        e = x1[a:b].T @ x2[a:b]
        t = (e.max(dim=1, keepdim=True)[0] - e) if max_minus else e
        if live < c:                                        # (the row maximum of the max-minus form still sees every column)
            t = t.clone()
            t[:, live:] = -float("inf")
        att = torch.softmax(t, dim=1)
        d_a = value[a:b].T @ g_out[a:b]
        d_t = att * (d_a - (d_a * att).sum(dim=1, keepdim=True))
        d_e = -d_t if (max_minus and defect != 10) else d_t
        out["out"][a:b] = value[a:b] @ att
        out["dvalue"][a:b] = g_out[a:b] @ (att if defect == 9 else att.T)
        out["dx1"][a:b] = x2[a:b] @ d_e.T
        out["dx2"][a:b] = x1[a:b] @ d_e
    return out
