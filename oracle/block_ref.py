"""oracle/block_ref.py -- TEST INFRASTRUCTURE ONLY.

Dtype-agnostic restatement of the two units weasal_amd/csrc/blocks.hip composes (ws_kpblock_fwd / _bwd, ws_upunary_fwd /
_bwd), built from the functions of oracle/kpconv_ref.py, with gradients from torch autograd on leaves of the requested
dtype; a case table; a case builder that avoids LeakyReLU sign flips by construction; and a plain-Python ledger of the
predicates the block calls branch on.  Used by tests/test_block_branches_cpu.py and tests/test_block_branches_gpu.py.

Units
  kpblock_ref   [unary1 ->] gather -> contraction with wk -> bias -> LeakyReLU [-> unary2 + shortcut -> LeakyReLU]; the shortcut
                is the input rows, their max-pool over the index rows (strided), or either projected (ws, with its bias bs).
  upunary_ref   nearest upsample of column 0 of `ups` (the shadow index reads a zero row) -> concat(skip) -> linear + bias
                -> [LeakyReLU] -> [dropout: keep bits of oracle.gemm_branch_ref.drop_keep at row * out_dim + col].

Descriptor flags, as the reference models them
  dout_pregated      the reference backpropagates the upstream gradient g; the device is handed g * where(out_ref64 > 0, 1, slope)
                     (times keep * scale for a decoder step with dropout: what the consumer's gate leaves, GateLink.drop).
  gate_dfeat / _dxc  the expected input gradient is the reference's times where(input > 0, 1, slope): strictly, so the 0.0 and
                     -0.0 the gated cases carry in their inputs take the slope.
  dfeat_add          added to the reference's input gradient before the gate.

Case builder.  One LeakyReLU pre-activation that rounds to the other side of zero moves a gradient element by 90 %.  A case
is evaluated in float64 and in float32 on the CPU; per stage e32 = max |z32 - z64|; the case is *decided* when every
pre-activation of every stage has |z64| >= 16 e32 + 4e-6 max |z64| (four times the comparison bound).  The builder takes the
first decided data seed at or after the case's base seed, at most 64 tries; the geometry is drawn once per case.  Nothing is
masked or excluded.  Inputs come from a CPU generator, so a seed means the same tensors everywhere; WHICH seed is the first
decided one follows the float32 library of the machine that runs the test (one case moved by three seeds between two hosts),
and reference and device always see the seed chosen there.  A pooled maximum that is an exact tie between two real rows is refused (assert); a tie with the shadow
row's zero is routed to the first column on both sides (torch.max and the kernels: "first maximum wins").

Bound, per tensor (tests/test_attention_gpu.py's, for its reason: the yardstick is the float32 arithmetic the calls replace)
    max |device - ref64|  <=  FACTOR * max |ref32 - ref64|  +  1e-6 * max |ref64|,     FACTOR = 4 for every tensor.
No tensor needed a factor of its own: the largest measured ratio to this bound is 0.44 (an output), 0.28 for a gradient.
"""
import types

import torch

from . import kpconv_ref as R
from .gemm_branch_ref import drop_args, drop_keep

SLOPE = 0.1
FACTOR = 4.0
FLOOR = 1e-6
TRIES = 64
NO_LIMIT = 1 << 62            # ws_block_group_rows at its default
DROP_SEED = 424242
SWITCHES = ("ws_block_gates", "ws_block_packed_k4", "ws_block_pool_order", "ws_block_group_rows", "ws_block_gather_residual",
            "ws_block_fused_infer")


def lrelu(z):
    return torch.nn.functional.leaky_relu(z, SLOPE)


def gate_of(x):
    """LeakyReLU'(x) as the gates decide it: strictly x > 0"""
    return torch.where(x > 0, torch.ones_like(x), torch.full_like(x, SLOPE))


# ----------------------------------------------------------------------------------------------------------------------
# case tables
# ----------------------------------------------------------------------------------------------------------------------
def _kp(name, base_seed, kind="resnet", in_dim=64, conv=32, out_dim=128, w1=True, ws=True, strided=False, ns=128, nq=None,
        K=15, bias=False, want_dfeat=True, dfeat_add=False, gate_dfeat=False, dout_pregated=False, offset=None, wide_inds=False,
        infer=False, rows_sorted=False, switches=None, geometry="cpu", shadow_row=False, zeros=False, orders=False):
    if kind == "simple":
        conv_in, conv_out, w1, ws = in_dim, out_dim, False, False
    else:
        conv_in = conv_out = conv
        assert w1 or in_dim == conv
        assert ws or in_dim == out_dim
    return types.SimpleNamespace(
        unit="kp", name=name, base_seed=base_seed, kind=kind, in_dim=in_dim, conv_in=conv_in, conv_out=conv_out, out_dim=out_dim,
        w1=w1, ws=ws, strided=strided, ns=ns, nq=(ns // 3 if strided else ns) if nq is None else nq, K=K, bias=bias,
        want_dfeat=want_dfeat and not infer, dfeat_add=dfeat_add, gate_dfeat=gate_dfeat, dout_pregated=dout_pregated, offset=offset,
        wide_inds=wide_inds, infer=infer, rows_sorted=rows_sorted, switches=dict(switches or {}), geometry=geometry,
        shadow_row=shadow_row, zeros=zeros or gate_dfeat, orders=orders)


KP_CASES = [
    # widths in -> out (resnet: conv = out / 4 both ways)
    _kp("simple_64_128", 100, kind="simple", in_dim=64, out_dim=128, ns=160),
    _kp("simple_first_block_bias", 110, kind="simple", in_dim=16, out_dim=64, bias=True, want_dfeat=False, ns=96),
    _kp("simple_gate_feat", 120, kind="simple", in_dim=32, out_dim=64, gate_dfeat=True, ns=128),
    _kp("simple_pregated", 130, kind="simple", in_dim=32, out_dim=64, dout_pregated=True, ns=128),
    _kp("simple_pregated_bias", 140, kind="simple", in_dim=32, out_dim=64, dout_pregated=True, bias=True, ns=128),
    _kp("resnet_64_128", 200, ns=192),
    _kp("resnet_64_128_bias", 210, ns=192, bias=True, shadow_row=True),
    _kp("resnet_16_64_bias", 220, in_dim=16, conv=16, out_dim=64, bias=True, ns=128),
    _kp("resnet_w1_offset", 230, offset="w1", ns=128),
    _kp("resnet_identity_128", 240, in_dim=128, conv=32, out_dim=128, ws=False, ns=128),
    _kp("resnet_no_unary1_32_128", 250, in_dim=32, conv=32, out_dim=128, w1=False, ns=128),
    _kp("resnet_no_unary1_first_block", 260, in_dim=32, conv=32, out_dim=128, w1=False, want_dfeat=False, ns=96),
    _kp("resnet_first_block", 270, want_dfeat=False, ns=128),
    _kp("resnet_add_trailing", 280, dfeat_add=True, ns=128),
    _kp("resnet_gate_unary1", 290, gate_dfeat=True, ns=128),
    _kp("resnet_pregated", 300, dout_pregated=True, ns=128),
    _kp("resnet_pregated_bias", 310, dout_pregated=True, bias=True, ns=128),
    _kp("resnet_rows_sorted", 320, rows_sorted=True, ns=128),
    _kp("resnet_grid", 330, geometry="pyramid"),
    _kp("strided_projection", 400, strided=True, ns=192, orders=True),
    _kp("strided_projection_bias", 410, strided=True, ns=192, bias=True, orders=True, shadow_row=True),
    _kp("strided_identity_128", 420, strided=True, in_dim=128, conv=32, out_dim=128, ws=False, ns=192, orders=True),
    _kp("strided_wide_inds", 430, strided=True, ns=192, wide_inds=True, orders=True),
    _kp("strided_feat_offset_add", 440, strided=True, in_dim=16, conv=16, out_dim=64, bias=True, ns=192, offset="feat", dfeat_add=True),
    _kp("strided_add_bytes", 450, strided=True, ns=192, dfeat_add=True, orders=True),
    _kp("strided_add_gate", 460, strided=True, ns=192, dfeat_add=True, gate_dfeat=True, orders=True),
    _kp("strided_wide_inds_add", 470, strided=True, ns=192, wide_inds=True, dfeat_add=True),
    _kp("infer_one_launch", 500, infer=True, ns=128),
    _kp("infer_two_launches", 510, infer=True, ns=128, switches={"ws_block_fused_infer": 0}),
    _kp("infer_k9", 520, infer=True, K=9, ns=128),
    _kp("infer_k13", 530, infer=True, K=13, kind="simple", in_dim=32, out_dim=32, ns=128),
    _kp("switch_gates_0", 600, ns=128, switches={"ws_block_gates": 0}),
    _kp("switch_packed_k4_0", 610, strided=True, ns=192, switches={"ws_block_packed_k4": 0}, orders=True),
    _kp("switch_pool_order_0", 620, strided=True, ns=192, switches={"ws_block_pool_order": 0}, orders=True),
    _kp("switch_group_rows_0", 630, ns=192, switches={"ws_block_group_rows": 0}),
    # unary1 and the shortcut projection of the same width: the pair shares an instantiation, so it is ONE launch where it groups
    _kp("resnet_64_32_32", 340, in_dim=64, conv=32, out_dim=32, ns=192),
    _kp("switch_group_rows_0_64_32_32", 650, in_dim=64, conv=32, out_dim=32, ns=192, switches={"ws_block_group_rows": 0}),
    _kp("switch_group_rows_0_strided", 640, strided=True, ns=192, dfeat_add=True, switches={"ws_block_group_rows": 0}, orders=True),
]


def _up(name, base_seed, widths="A", relu=True, bias=True, drop=0.0, dout_pregated=False, gate_dxc=False, switches=None):
    c_up, c_skip, out_dim = {"A": (64, 32, 32), "B": (128, 128, 64)}[widths]
    return types.SimpleNamespace(unit="up", name=name, base_seed=base_seed, nc=37, nf=300, c_up=c_up, c_skip=c_skip, out_dim=out_dim,
                                 relu=relu, bias=bias, drop=drop, dout_pregated=dout_pregated, gate_dxc=gate_dxc,
                                 switches=dict(switches or {}))


UP_CASES = [
    _up("up_relu_bias", 700),
    _up("up_relu", 710, widths="B", bias=False),
    _up("up_linear_bias", 720, relu=False),
    _up("up_linear", 730, widths="B", relu=False, bias=False),
    _up("up_dropout", 740, widths="B", drop=0.5),
    _up("up_dropout_pool_first", 750, drop=0.5, switches={"ws_block_gather_residual": 0}),
    _up("up_pool_first", 760, switches={"ws_block_gather_residual": 0}),
    _up("up_pregated_bias", 770, dout_pregated=True),
    _up("up_pregated", 780, widths="B", bias=False, dout_pregated=True),
    _up("up_dropout_pregated", 790, widths="B", drop=0.5, dout_pregated=True),
    _up("up_gate_dxc", 800, gate_dxc=True),
    _up("up_switch_group_rows_0", 810, widths="B", bias=False, switches={"ws_block_group_rows": 0}),      # (up_relu's shape)
]

CASES = {c.name: c for c in KP_CASES + UP_CASES}
assert len(CASES) == len(KP_CASES) + len(UP_CASES)


# ----------------------------------------------------------------------------------------------------------------------
# geometry (CPU generator: a function of the case alone)
# ----------------------------------------------------------------------------------------------------------------------
CONV_RADIUS = 1.0


def kernel_points(K, radius=CONV_RADIUS):
    """a centre point and K - 1 points at 0.4 .. 0.66 of the radius (the reach the sorted-row cutoff assumes: < 0.7)"""
    g = torch.Generator().manual_seed(9000 + K)
    v = torch.randn(K, 3, generator=g)
    v = v / v.norm(dim=1, keepdim=True) * (0.4 + 0.26 * torch.rand(K, 1, generator=g)) * radius
    v[0] = 0.0
    return v.float()


def radius_rows(q, s, radius):
    """index rows of a brute-force radius search, sorted by distance, padded with the shadow index ns (float64 distances)"""
    d2 = ((q.double()[:, None, :] - s.double()[None, :, :]) ** 2).sum(2)
    ns = s.shape[0]
    inside = d2 < radius * radius
    width = int(inside.sum(1).max())
    d2 = torch.where(inside, d2, torch.full_like(d2, float("inf")))
    order = torch.argsort(d2, dim=1, stable=True)[:, :width]
    return torch.where(torch.gather(inside, 1, order), order, torch.full_like(order, ns)).contiguous()


def kp_geometry(c):
    assert c.geometry == "cpu"
    g = torch.Generator().manual_seed(50000 + c.base_seed)
    search = CONV_RADIUS * (1.5 if c.rows_sorted else 1.0)
    per_ball = 30.0 if c.rows_sorted else 16.0
    side = search * (c.ns * 4.19 / per_ball) ** (1.0 / 3.0)
    s = (torch.rand(c.ns, 3, generator=g) * side).float()
    q = s[::c.ns // c.nq][:c.nq].contiguous() if c.strided else s
    assert q.shape[0] == c.nq
    inds = radius_rows(q, s, search)
    if c.wide_inds:
        inds = torch.cat([inds, torch.full((c.nq, 256 - inds.shape[1]), c.ns, dtype=inds.dtype)], 1).contiguous()
    if c.shadow_row:
        # a query without a single real neighbour (in cases with biases: without them its pre-activations are exact zeros,
        # which both sides compute exactly but the builder's rule cannot call decided)
        inds[c.nq // 2, :] = c.ns
    return types.SimpleNamespace(q_pts=q, s_pts=s, inds=inds, kp=kernel_points(c.K), extent=0.48 * CONV_RADIUS, radius=CONV_RADIUS,
                                 search_radius=search)


def up_geometry(c):
    g = torch.Generator().manual_seed(50000 + c.base_seed)
    ups = torch.randint(0, c.nc, (c.nf, 3), generator=g)
    ups[::17, 0] = c.nc                         # shadow rows: the zero feature
    return types.SimpleNamespace(ups=ups.contiguous())


# ----------------------------------------------------------------------------------------------------------------------
# inputs (float32, CPU generator)
# ----------------------------------------------------------------------------------------------------------------------
def _zeros_into(x):
    """exact 0.0 and -0.0 in a few elements, each in a column of its own"""
    x[1, 0] = 0.0
    x[2, 1] = -0.0
    x[5, 3] = 0.0
    x[x.shape[0] - 1, 2] = -0.0


def kp_inputs(c, seed, geo):
    g = torch.Generator().manual_seed(seed)
    ns, nq = geo.s_pts.shape[0], geo.q_pts.shape[0]

    def n(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).float()
    t = {"feat": n(ns, c.in_dim)}
    if c.zeros:
        _zeros_into(t["feat"])
        if c.strided and c.kind == "resnet":
            # a pooled maximum that is an exact tie of a real 0.0 (support 1, column 0) with the shadow row's zero: every other
            # real neighbour of one padded query row is negative there
            rows = ((geo.inds == 1).any(1) & (geo.inds == ns).any(1)).nonzero().flatten()
            assert rows.numel() > 0, "no padded query row holds support 1"
            js = geo.inds[int(rows[0])]
            js = js[(js != ns) & (js != 1)]
            t["feat"][js, 0] = -t["feat"][js, 0].abs()
    t["w1"] = n(c.conv_in, c.in_dim, scale=c.in_dim ** -0.5) if c.w1 else None
    t["wk"] = n(c.K, c.conv_in, c.conv_out, scale=(c.K * c.conv_in / 4.0) ** -0.5)
    resnet = c.kind == "resnet"
    t["w2"] = n(c.out_dim, c.conv_out, scale=c.conv_out ** -0.5) if resnet else None
    t["ws"] = n(c.out_dim, c.in_dim, scale=c.in_dim ** -0.5) if c.ws else None
    t["b1"] = n(c.conv_in, scale=0.1) if (c.bias and c.w1) else None
    t["bk"] = n(c.conv_out, scale=0.1) if c.bias else None
    t["b2"] = n(c.out_dim, scale=0.1) if (c.bias and resnet) else None
    t["bs"] = n(c.out_dim, scale=0.1) if (c.bias and c.ws) else None
    t["g"] = n(nq, c.out_dim)
    t["dfeat_add"] = n(ns, c.in_dim) if c.dfeat_add else None
    return t


def up_inputs(c, seed, geo):
    g = torch.Generator().manual_seed(seed)

    def n(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).float()
    t = {"xc": n(c.nc, c.c_up), "skip": n(c.nf, c.c_skip)}
    if c.gate_dxc:
        _zeros_into(t["xc"])
    t["w"] = n(c.out_dim, c.c_up + c.c_skip, scale=(c.c_up + c.c_skip) ** -0.5)
    t["b"] = n(c.out_dim, scale=0.1) if c.bias else None
    t["g"] = n(c.nf, c.out_dim)
    return t


# ----------------------------------------------------------------------------------------------------------------------
# the two units
# ----------------------------------------------------------------------------------------------------------------------
def _leaf(t, dtype, grad=True):
    return None if t is None else t.detach().to(dtype).clone().requires_grad_(grad)


def _straight_through(z, y):
    """y forward, identity backward: what a skipped activation-backward pass computes"""
    return z + (y - z).detach()


def kpblock_ref(c, geo, t, dtype, remove=None, grads=True):
    """-> {"out", "pre": {stage: pre-activation}, and with grads: dfeat, dw1, db1, dwk, dbk, dw2, db2, dws, dbs} (None where absent).
    remove: one effect taken out -- "dfeat_add", "gate", "pregating", "shortcut", "bias:<name>"."""
    q, s, kp = geo.q_pts.to(dtype), geo.s_pts.to(dtype), geo.kp.to(dtype)
    inds = geo.inds
    names = ("feat", "w1", "b1", "wk", "bk", "w2", "b2", "ws", "bs")
    L = {k: _leaf(t[k], dtype, grads) for k in names}
    if remove and remove.startswith("bias:"):
        L[remove[5:]] = torch.zeros_like(L[remove[5:]])
    feat, pre = L["feat"], {}
    x = feat
    if L["w1"] is not None:
        pre["unary1"] = R.matmul_epilogue_ref(feat, L["w1"].t(), bias=L["b1"])
        x = lrelu(pre["unary1"])
    wf, _ = R.kpconv_gather_ref(x, q, s, inds, kp, geo.extent)
    pre["conv"] = R.matmul_epilogue_ref(wf.reshape(wf.shape[0], -1), L["wk"].reshape(-1, c.conv_out), bias=L["bk"])
    out = lrelu(pre["conv"])
    last = "conv"
    if L["w2"] is not None:
        sc = R.max_pool_ref(feat, inds) if c.strided else feat
        if L["ws"] is not None:
            sc = R.matmul_epilogue_ref(sc, L["ws"].t(), bias=L["bs"])
        if remove == "shortcut":
            sc = None
        pre["unary2"] = R.matmul_epilogue_ref(out, L["w2"].t(), bias=L["b2"], residual=sc)
        out = lrelu(pre["unary2"])
        last = "unary2"
    res = {"out": out.detach(), "pre": {k: v.detach() for k, v in pre.items()}}
    if not grads:
        return res
    if remove == "pregating":
        out = _straight_through(pre[last], out)
    out.backward(t["g"].to(dtype))
    for k in names[1:]:
        res["d" + k] = None if (L[k] is None or not L[k].requires_grad) else L[k].grad
    dfeat = None
    if c.want_dfeat:
        dfeat = feat.grad
        if c.dfeat_add and remove != "dfeat_add":
            dfeat = dfeat + t["dfeat_add"].to(dtype)
        if c.gate_dfeat and remove != "gate":
            dfeat = dfeat * gate_of(feat.detach())
    res["dfeat"] = dfeat
    return res


def keep_mask(c):
    """[nf, out_dim] bool keep bits of the decoder step's dropout (the device hash)"""
    return torch.from_numpy(drop_keep(DROP_SEED, c.drop, c.nf, c.out_dim, c.out_dim))


def upunary_ref(c, geo, t, dtype, remove=None, grads=True):
    """-> {"out", "pre", and with grads: dxc, dskip, dw, db}.  remove: "shadow", "dropout", "gate", "pregating", "bias:b"."""
    L = {k: _leaf(t[k], dtype, grads) for k in ("xc", "skip", "w", "b")}
    if remove == "bias:b":
        L["b"] = torch.zeros_like(L["b"])
    ups = geo.ups
    if remove == "shadow":
        ups = torch.where(ups >= c.nc, torch.zeros_like(ups), ups)         # the shadow index reads a real row
    up = R.closest_pool_ref(L["xc"], ups)
    z = R.matmul_epilogue_ref(torch.cat([up, L["skip"]], 1), L["w"].t(), bias=L["b"])
    pre = {"unary": z} if c.relu else {}
    act = lrelu(z) if c.relu else z
    out = act
    if c.drop > 0 and remove != "dropout":
        scale = drop_args(c.drop)[1]
        out = torch.where(keep_mask(c), act * scale, torch.zeros_like(act))
    res = {"out": out.detach(), "pre": {k: v.detach() for k, v in pre.items()}}
    if not grads:
        return res
    if remove == "pregating":
        out = _straight_through(z, out)
    out.backward(t["g"].to(dtype))
    dxc = L["xc"].grad
    if c.gate_dxc and remove != "gate":
        dxc = dxc * gate_of(L["xc"].detach())
    res.update(dxc=dxc, dskip=L["skip"].grad, dw=L["w"].grad, db=None if L["b"] is None or not L["b"].requires_grad else L["b"].grad)
    return res


def unit_ref(c, geo, t, dtype, remove=None, grads=True):
    return (kpblock_ref if c.unit == "kp" else upunary_ref)(c, geo, t, dtype, remove, grads)


def tensor_names(c):
    """the tensors a case compares"""
    if c.unit == "up":
        return ["out", "dxc", "dskip", "dw"] + (["db"] if c.bias else [])
    if c.infer:
        return ["out"]
    resnet = c.kind == "resnet"
    names = ["out", "dwk"] + (["dfeat"] if c.want_dfeat else [])
    names += ["dw1"] if c.w1 else []
    names += ["dw2"] if resnet else []
    names += ["dws"] if c.ws else []
    if c.bias:
        names += ["dbk"] + (["db1"] if c.w1 else []) + (["db2"] if resnet else []) + (["dbs"] if c.ws else [])
    return names


def device_dout(c, t, out64):
    """the float32 gradient the device is handed: g, or g with the consumer's gate applied (dout_pregated)"""
    g = t["g"].double()
    if c.dout_pregated:
        g = g * gate_of(out64)
        if c.unit == "up" and c.drop > 0:
            g = g * keep_mask(c).double() * drop_args(c.drop)[1]
    return g.float()


# ----------------------------------------------------------------------------------------------------------------------
# the builder
# ----------------------------------------------------------------------------------------------------------------------
def undecided(pre64, pre32):
    """names of the stages with a pre-activation closer to zero than 16 e32 + 4e-6 max |z64|"""
    bad = []
    for k, z64 in pre64.items():
        e32 = float((pre32[k].double() - z64).abs().max())
        if float(z64.abs().min()) < 16.0 * e32 + 4e-6 * float(z64.abs().max()):
            bad.append(k)
    return bad


def pool_ties(c, geo, t):
    """pooled maxima that are exact ties between two REAL rows (the shadow row's zero is no real row)"""
    if not (c.unit == "kp" and c.strided and c.kind == "resnet"):
        return 0
    ns = geo.s_pts.shape[0]
    x = torch.cat([t["feat"], torch.full((1, c.in_dim), float("-inf"))])[geo.inds]          # [nq, h, c]
    top = torch.topk(x, 2, dim=1).values
    return int(((top[:, 0] == top[:, 1]) & torch.isfinite(top[:, 0])).sum())


def shadow_pool_wins(c, geo, t):
    """pooled elements whose maximum is the shadow row's zero (no real value above it; an exact real 0.0 ties with it)"""
    if not (c.unit == "kp" and c.strided and c.kind == "resnet"):
        return 0, 0
    real = torch.cat([t["feat"], torch.full((1, c.in_dim), float("-inf"))])[geo.inds].max(1).values
    padded = (geo.inds == geo.s_pts.shape[0]).any(1, keepdim=True)
    return int(((real < 0) & padded).sum()), int(((real == 0) & padded).sum())


_BUILT = {}


def build(name, geo=None):
    """the case `name` at its first decided seed: inputs, float64 and float32 references, per-tensor float32 error.
    geo: the geometry of a case that takes it from elsewhere (geometry == "pyramid"); cached per name."""
    if name in _BUILT:
        return _BUILT[name]
    c = CASES[name]
    if geo is None:
        geo = kp_geometry(c) if c.unit == "kp" else up_geometry(c)
    make = kp_inputs if c.unit == "kp" else up_inputs
    log = []
    for seed in range(c.base_seed, c.base_seed + TRIES):
        t = make(c, seed, geo)
        f64 = unit_ref(c, geo, t, torch.float64, grads=False)
        f32 = unit_ref(c, geo, t, torch.float32, grads=False)
        bad = undecided(f64["pre"], f32["pre"])
        if not bad:
            break
        log.append((seed, bad))
    else:
        raise AssertionError("case %s: no decided seed in %d tries from %d: %s" % (name, TRIES, c.base_seed, log[-3:]))
    ties = pool_ties(c, geo, t)
    assert ties == 0, "case %s seed %d: %d pooled maxima tie between two real rows" % (name, seed, ties)
    r64 = unit_ref(c, geo, t, torch.float64)
    r32 = unit_ref(c, geo, t, torch.float32)
    names = tensor_names(c)
    err32 = {k: float((r32[k].double() - r64[k]).abs().max()) for k in names}
    b = types.SimpleNamespace(case=c, seed=seed, tries=seed - c.base_seed + 1, geo=geo, inputs=t, ref64=r64, ref32=r32, names=names,
                              err32=err32, dout=device_dout(c, t, r64["out"]))
    _BUILT[name] = b
    return b


def bound(b, key, factor=FACTOR):
    return factor * b.err32[key] + FLOOR * float(b.ref64[key].abs().max())


def ratios(b, got):
    """{tensor: (max |got - ref64|, bound, ratio)}; got: {tensor: float32 tensor (any device)}"""
    out = {}
    for k in b.names:
        err = float((got[k].detach().double().cpu() - b.ref64[k]).abs().max())
        bd = bound(b, k)
        out[k] = (err, bd, err / bd if bd > 0 else (0.0 if err == 0 else float("inf")))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# sensitivity: what a case turns on must leave a trace far above the bound
# ----------------------------------------------------------------------------------------------------------------------
def effects(c):
    """[(effect to remove, the tensor it must move)] of one case"""
    e = []
    if c.unit == "kp":
        if c.dfeat_add:
            e.append(("dfeat_add", "dfeat"))
        if c.gate_dfeat:
            e.append(("gate", "dfeat"))
        if c.dout_pregated:
            e.append(("pregating", "dw2" if c.kind == "resnet" else "dwk"))
        if c.ws:
            e.append(("shortcut", "out"))
        if c.bias:
            e += [("bias:bk", "out")] + ([("bias:b1", "out")] if c.w1 else [])
            e += [("bias:b2", "out")] if c.kind == "resnet" else []
            e += [("bias:bs", "out")] if c.ws else []
    else:
        e.append(("shadow", "out"))
        if c.drop > 0:
            e.append(("dropout", "out"))
        if c.gate_dxc:
            e.append(("gate", "dxc"))
        if c.dout_pregated:
            e.append(("pregating", "dw"))
        if c.bias:
            e.append(("bias:b", "out"))
    return e


def sensitivity(b):
    """{effect: (movement of its tensor, 100 x bound)}"""
    c = b.case
    out = {}
    for effect, key in effects(c):
        grads = key != "out"
        alt = unit_ref(c, b.geo, b.inputs, torch.float64, remove=effect, grads=grads)
        out[effect] = (float((alt[key] - b.ref64[key]).abs().max()), 100.0 * bound(b, key))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# branch ledger: the predicates of blocks.hip from a case's shapes and flags
# ----------------------------------------------------------------------------------------------------------------------
def _grouped(c, rows):
    limit = c.switches.get("ws_block_group_rows", NO_LIMIT)
    return limit > 0 and 0 < rows < limit


def _in_place(k, n, offset=False):
    """Lin::in_place of a contiguous weight (ldw = k): k % 32, n % 4, the pointer's 16-byte alignment"""
    return "yes" if (k % 32 == 0 and n % 4 == 0 and not offset) else ("no: alignment" if (k % 32 == 0 and n % 4 == 0) else "no: shape")


def kp_ledger(c, h=None):
    """h: the width of the case's index matrix (the arg record's rule); None: 256 for the wide cases, narrow otherwise"""
    led = {}
    gates = c.switches.get("ws_block_gates", 1)
    resnet = c.kind == "resnet"
    h = (256 if c.wide_inds else 16) if h is None else h
    kc = c.K * c.conv_in
    l1 = _in_place(c.in_dim, c.conv_in, c.offset == "w1") if c.w1 else None
    lsc = _in_place(c.in_dim, c.out_dim) if c.ws else None
    led["block"] = (("resnet" if c.w1 else "resnet without unary1") + (", projection" if c.ws else ", identity shortcut")) if resnet else "simple"
    led["strided"] = ("strided, projection" if c.ws else "strided, pooled rows as residual") if (c.strided and resnet) else "no"
    led["in_place unary1"] = l1
    led["in_place unary2"] = _in_place(c.conv_out, c.out_dim) if resnet else None
    led["in_place shortcut"] = lsc
    led["biases"] = c.bias
    led["rows_sorted"] = c.rows_sorted
    led["pair_in"] = bool(_grouped(c, c.nq) and c.w1 and resnet and c.ws and not c.strided and l1 == "yes" and lsc == "yes") if resnet else None
    arg_bytes = (h <= 255 and c.in_dim % 4 == 0 and c.offset != "feat") if (c.strided and resnet) else None
    led["arg_bytes"] = arg_bytes
    if c.infer:
        led["forward"] = "one launch" if (c.K == 15 and c.conv_in == 32 and c.conv_out == 32 and not c.rows_sorted
                                          and c.switches.get("ws_block_fused_infer", 1)) else "forward only: gather + product"
        return led
    led["forward"] = "training: gather + product"
    need_dx1 = c.want_dfeat or c.w1
    want_sc = resnet and c.want_dfeat
    grp = _grouped(c, max(c.nq, c.ns))
    led["grouped leaves"] = grp
    led["need_dx1"] = need_dx1
    led["want_sc"] = want_sc if resnet else None
    led["in_place wk^T"] = _in_place(c.conv_out, kc) if need_dx1 else None
    led["pair_dz"] = bool(grp and want_sc and c.ws) if resnet else None
    led["gated2"] = bool(not c.bias and gates) if resnet else None
    led["dout_pregated"] = ("resnet" if resnet else "simple") if c.dout_pregated else "no"
    if need_dx1:
        gate1 = "x1" if (c.w1 and not c.bias and gates) else ("feat" if (not c.w1 and c.gate_dfeat and c.want_dfeat) else "none")
        led["gate1"] = gate1
        if c.geometry == "pyramid" and not c.strided:
            led["route"] = "slab grid"
        else:
            led["route"] = "table, packed entry" if c.switches.get("ws_block_packed_k4", 1) else "table, gated entry"
    led["gate_dfeat"] = (("unary1 product's epilogue" if c.w1 else "K4 store") + (", after dfeat_add" if c.dfeat_add else "")) if c.gate_dfeat else "no"
    if c.dfeat_add:
        led["dfeat_add"] = ("pool backward's store" if arg_bytes else "add_rows after the int32 pool") if (c.strided and want_sc) else "trailing pass"
    else:
        led["dfeat_add"] = "none"
    if c.want_dfeat:
        led["dfeat written by"] = "unary1 product" if c.w1 else ("K4 + shortcut rows" if resnet else "K4")
    else:
        led["dfeat written by"] = "not wanted"
    return led


def up_ledger(c):
    led = {}
    if c.relu and c.dout_pregated:
        led["activation backward"] = "pregated"
    elif c.drop > 0:
        led["activation backward"] = "LeakyReLU' and dropout"
    elif c.relu:
        led["activation backward"] = "LeakyReLU'"
    else:
        led["activation backward"] = "linear"
    if c.switches.get("ws_block_gather_residual", 1):
        led["forward epilogue"] = "gathered residual"
    else:
        led["forward epilogue"] = "pool first, dropout epilogue" if c.drop > 0 else "pool first, plain epilogue"
    led["db"] = c.bias
    led["relu"] = c.relu
    led["dropout"] = c.drop > 0
    led["gate_dxc"] = c.gate_dxc
    led["dout_pregated"] = c.dout_pregated
    led["grouped leaves"] = _grouped(c, max(c.nc, c.nf))
    led["widths"] = "%d/%d->%d" % (c.c_up, c.c_skip, c.out_dim)
    return led


def ledger(c, **kw):
    return kp_ledger(c, **kw) if c.unit == "kp" else up_ledger(c)


# every value every predicate must take somewhere in the case table
KP_REQUIRED = {
    "block": {"simple", "resnet, projection", "resnet, identity shortcut", "resnet without unary1, projection"},
    "strided": {"no", "strided, projection", "strided, pooled rows as residual"},
    "in_place unary1": {"yes", "no: shape", "no: alignment"},
    "in_place unary2": {"yes", "no: shape"},
    "in_place shortcut": {"yes", "no: shape"},
    "in_place wk^T": {"yes", "no: shape"},
    "biases": {True, False},
    "rows_sorted": {True, False},
    "pair_in": {True, False},
    "pair_dz": {True, False},
    "grouped leaves": {True, False},
    "arg_bytes": {True, False},
    "forward": {"one launch", "forward only: gather + product", "training: gather + product"},
    "need_dx1": {True, False},
    "want_sc": {True, False},
    "gated2": {True, False},
    "gate1": {"x1", "feat", "none"},
    "dout_pregated": {"no", "resnet", "simple"},
    "route": {"slab grid", "table, packed entry", "table, gated entry"},
    "gate_dfeat": {"no", "unary1 product's epilogue", "K4 store", "unary1 product's epilogue, after dfeat_add"},
    "dfeat_add": {"none", "pool backward's store", "add_rows after the int32 pool", "trailing pass"},
    "dfeat written by": {"unary1 product", "K4 + shortcut rows", "K4", "not wanted"},
}
UP_REQUIRED = {
    "activation backward": {"pregated", "LeakyReLU' and dropout", "LeakyReLU'", "linear"},
    "forward epilogue": {"gathered residual", "pool first, dropout epilogue", "pool first, plain epilogue"},
    "db": {True, False},
    "relu": {True, False},
    "dropout": {True, False},
    "gate_dxc": {True, False},
    "dout_pregated": {True, False},
    "grouped leaves": {True, False},
    "widths": {"64/32->32", "128/128->64"},
}


def coverage(cases, required):
    """{predicate: the required values no case takes}"""
    seen = {k: set() for k in required}
    for c in cases:
        for k, v in ledger(c).items():
            if k in seen and v is not None:
                seen[k].add(v)
    return {k: sorted(map(str, required[k] - seen[k])) for k in required if required[k] - seen[k]}
