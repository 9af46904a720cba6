"""Evaluation-mode batch normalisation folded into the product in front of it, restated (the contract of ws_bn_fold_fwd /
ws_bn_fold_bwd, include/weasal_hip.h).

A site is a weight seen as [outer, c, inner] with the BN channel on the middle axis, gamma, beta, running_mean, running_var
[c] and eps:

  forward   rstd = 1 / sqrt(var + eps),  a = gamma rstd,  w_out = a w (along the middle axis),  t_out = beta - mean a
  backward  dw = a dw_out,  dbeta = dt_out,  dgamma_c = rstd_c (sum over outer, inner of dw_out w  -  mean_c dt_out_c);
            dw_out / dt_out None stand for zeros

Everything runs on the CPU in the dtype asked for; float64 is the reference.  The kernels are float32 with every operation
rounded on its own, so the bounds count roundings (u = 2^-24, one ulp <= 2 u relative = 2^-23):

  w_out   five individually rounded operations.  rstd is three of them: the sum var + eps (half an ulp, which the square
          root halves), sqrtf and the division, each allowed a whole ulp on the device: 0.25 + 1 + 1; a = gamma * rstd adds
          half an ulp and w_out = a * w another: at most 3.25 ulp, held to 4 * 2^-23 |ref|
  t_out   one more product (mean * a) and one sum: 5 * 2^-23 (|beta| + |mean a|)
  dw      as w_out: 4 * 2^-23 |ref|
  dgamma  a float32 sum of L = outer * inner individually rounded products in ANY order, the product mean * dt, the
          difference and the product with rstd: (L + 8) u (sum |dw_out w| + |mean dt|) rstd, plus the 4 * 2^-23 |ref| of rstd
  dbeta   the bits of dt_out

`mutation` turns the restatement into one of four WRONG ones (the negative control of tests/test_bn_fold_cpu.py).  ROWS is
the table both test files walk; `case(row_id)` builds a row's inputs and the float64 reference once and caches them.
"""
import functools

import torch

EPS = 1e-5
ULP = 2.0 ** -23
MUTATIONS = ("var_without_eps", "t_without_mean", "dgamma_without_mean_dt", "wrong_axis")
WS_BN_FOLD_MAX = 32


def _bc(v, dim=3):
    return v.view(1, -1, 1) if dim == 3 else v


def forward(w, gamma, beta, mean, var, eps=EPS, dtype=torch.float64, mutation=None):
    """w [outer, c, inner] -> dict(w_out, t_out, a, rstd)"""
    w, gamma, beta, mean, var = (t.to(dtype) for t in (w, gamma, beta, mean, var))
    rstd = 1 / torch.sqrt(var if mutation == "var_without_eps" else var + eps)
    a = gamma * rstd
    if mutation == "wrong_axis" and w.shape[0] * w.shape[2] > 1:
        # the scale taken along the flattened (outer, inner) index instead of the channel
        idx = torch.arange(w.shape[0] * w.shape[2]) % w.shape[1]
        w_out = (w.permute(1, 0, 2).reshape(w.shape[1], -1) * a[idx]).reshape(w.shape[1], w.shape[0], w.shape[2]).permute(1, 0, 2)
    else:
        w_out = w * _bc(a)
    t_out = beta.clone() if mutation == "t_without_mean" else beta - mean * a
    return {"w_out": w_out.contiguous(), "t_out": t_out, "a": a, "rstd": rstd}


def backward(w, gamma, mean, var, dw_out, dt_out, eps=EPS, dtype=torch.float64, mutation=None):
    """-> dict(dw, dgamma, dbeta) and the absolute sums the dgamma bound is made of (dgamma_abs)"""
    w, gamma, mean, var = (t.to(dtype) for t in (w, gamma, mean, var))
    g = torch.zeros_like(w) if dw_out is None else dw_out.to(dtype)
    dt = torch.zeros_like(gamma) if dt_out is None else dt_out.to(dtype)
    rstd = 1 / torch.sqrt(var + eps)
    a = gamma * rstd
    s = (g * w).sum(dim=(0, 2))
    md = 0 if mutation == "dgamma_without_mean_dt" else mean * dt
    return {"dw": g * _bc(a), "dgamma": rstd * (s - md), "dbeta": dt.clone(),
            "dgamma_abs": ((g * w).abs().sum(dim=(0, 2)) + (mean * dt).abs()) * rstd}


def violations(got, ref, ins):
    """[(tensor, worst excess over the bound)] of a result (any dtype) against the float64 reference `ref` of the inputs `ins`"""
    bad = []

    def hold(name, value, bound):
        value = value.double().cpu().reshape(ref[name].shape)
        err = (value - ref[name]).abs()
        over = err - bound
        if not bool(torch.isfinite(value).all()) or bool((over > 0).any()):
            bad.append((name, float(over.max()) if bool(torch.isfinite(over).all()) else float("inf")))

    if "w_out" in got:
        hold("w_out", got["w_out"], 4 * ULP * ref["w_out"].abs())
    if "t_out" in got:
        hold("t_out", got["t_out"], 5 * ULP * (ins["beta"].double().abs() + (ins["mean"].double() * ref["a"]).abs()))
    if "dw" in got:
        hold("dw", got["dw"], 4 * ULP * ref["dw"].abs())
    if "dgamma" in got:
        length = ins["w"].shape[0] * ins["w"].shape[2]
        hold("dgamma", got["dgamma"], (length + 8) * 2.0 ** -24 * ref["dgamma_abs"] + 4 * ULP * ref["dgamma"].abs())
    if "dbeta" in got:
        if not torch.equal(got["dbeta"].double().cpu(), ref["dbeta"]):
            bad.append(("dbeta", float((got["dbeta"].double().cpu() - ref["dbeta"]).abs().max())))
    return bad


# ------------------------------------------------------------------------------------------------------------------
# the rows: id, outer, c, inner, and what is special about them
# ------------------------------------------------------------------------------------------------------------------
def _row(rid, outer, c, inner, off=None, var_zero=False, big_mean=False, null=None):
    return {"id": rid, "outer": outer, "c": c, "inner": inner, "off": off, "var_zero": var_zero, "big_mean": big_mean, "null": null}


ROWS = []
for _c in (1, 3, 4, 32, 130):
    for _k in (1, 3, 32, 129):
        ROWS.append(_row("linear-c%d-k%d" % (_c, _k), 1, _c, _k))
for _K in (9, 15):
    for _ci in (1, 4, 32):
        for _co in (4, 32, 66):
            ROWS.append(_row("kpconv-K%d-ci%d-co%d" % (_K, _ci, _co), _K * _ci, _co, 1))
ROWS += [
    _row("linear-c32-k32-src-off", 1, 32, 32, off="src"),            # a pointer 4 bytes off: the scalar branch
    _row("linear-c32-k32-dst-off", 1, 32, 32, off="dst"),
    _row("kpconv-K15-ci4-co32-src-off", 60, 32, 1, off="src"),
    _row("kpconv-K15-ci4-co32-dst-off", 60, 32, 1, off="dst"),
    _row("linear-c32-k32-var0", 1, 32, 32, var_zero=True),           # only eps under the root
    _row("kpconv-K15-ci4-co32-var0", 60, 32, 1, var_zero=True),
    _row("linear-c32-k32-bigmean", 1, 32, 32, big_mean=True),        # |mean| / std = 1e3
    _row("kpconv-K15-ci4-co32-bigmean", 60, 32, 1, big_mean=True),
    _row("kpconv-K15-ci80-co32-tall", 1200, 32, 1),                  # >= 1024 rows: the narrow column tile
    _row("linear-c130-k2052-chunks", 1, 130, 2052),                  # many element chunks, rows longer than a wave's stride
    _row("mid-o3-c5-i7", 3, 5, 7),                                   # the general [outer, c, inner] form
    _row("linear-c32-k32-no-dw", 1, 32, 32, null="dw_out"),          # the bias-free use of a folded weight's transpose
    _row("kpconv-K15-ci4-co32-no-dw", 60, 32, 1, null="dw_out"),
    _row("linear-c32-k32-no-dt", 1, 32, 32, null="dt_out"),
    _row("kpconv-K15-ci4-co32-no-dt", 60, 32, 1, null="dt_out"),
]
BY_ID = {r["id"]: r for r in ROWS}
assert len(BY_ID) == len(ROWS)


def inputs(row, seed=None):
    """float32 inputs of a row: w, gamma, beta, mean, var, dw_out, dt_out (the last two None where the row says NULL)"""
    g = torch.Generator().manual_seed(1000 + ROWS.index(row) if seed is None else seed)
    outer, c, inner = row["outer"], row["c"], row["inner"]
    w = torch.randn(outer, c, inner, generator=g) * 0.3
    gamma = torch.rand(c, generator=g) + 0.5
    beta = torch.randn(c, generator=g) * 0.2
    var = torch.zeros(c) if row["var_zero"] else torch.rand(c, generator=g) * 2 + 0.25
    mean = torch.randn(c, generator=g) * 0.5
    if row["big_mean"]:
        mean = torch.sqrt(var) * 1e3 * torch.where(torch.rand(c, generator=g) < 0.5, -1.0, 1.0)
    dw_out = None if row["null"] == "dw_out" else torch.randn(outer, c, inner, generator=g)
    dt_out = None if row["null"] == "dt_out" else torch.randn(c, generator=g)
    return {"w": w, "gamma": gamma, "beta": beta, "mean": mean, "var": var, "dw_out": dw_out, "dt_out": dt_out}


def reference(ins, dtype=torch.float64, mutation=None):
    f = forward(ins["w"], ins["gamma"], ins["beta"], ins["mean"], ins["var"], EPS, dtype, mutation)
    b = backward(ins["w"], ins["gamma"], ins["mean"], ins["var"], ins["dw_out"], ins["dt_out"], EPS, dtype, mutation)
    return {**f, **b}


@functools.lru_cache(maxsize=None)
def case(row_id):
    """(inputs, float64 reference) of a row, built once"""
    ins = inputs(BY_ID[row_id])
    return ins, reference(ins)
