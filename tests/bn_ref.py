"""Batch normalisation over the points, restated (the contract of ws_bn_fwd / ws_bn_bwd, include/weasal_hip.h).

For y [N, C], gamma, beta [C], eps, optional residual [N, C], act (0 none, 1 LeakyReLU(slope)):

  training    mean_c = (1/N) sum_i y_ic,  var_c = (1/N) sum_i (y_ic - mean_c)^2 (biased),  rstd = 1 / sqrt(var + eps)
              xhat = (y - mean) rstd,  z = xhat gamma + beta (+ residual),  out = act(z)
              running_mean = (1 - m) running_mean + m mean,  running_var = (1 - m) running_var + m var N / (N - 1),
              num_batches_tracked += 1
  evaluation  the same with mean = running_mean, var = running_var, no side effects
  backward    dz = dout * (out > 0 ? 1 : slope) with the gate taken from a GIVEN `out` (dz = dout when act = 0);
              dbeta = sum_i dz, dgamma = sum_i dz xhat, dresidual = dz;
              training: dy = gamma rstd (dz - dbeta / N - xhat dgamma / N);  evaluation: dy = gamma rstd dz

Everything runs on the CPU in the dtype asked for: float64 is the reference, float32 the yardstick of the bound

    max |kernel - ref64|  <=  4 * max |bn_ref in float32 - ref64|  +  1e-6 * max |ref64|        (per tensor)

`mutation` turns the restatement into one of seven WRONG ones (the negative control of tests/test_batchnorm_cpu.py).
ROWS is the table both test files walk; `case(row_id)` builds a row's inputs and both references once and caches them.
"""
import functools

import torch

EPS = 1e-5
SLOPE = 0.1
MUTATIONS = ("unbiased_norm", "raw_moments", "gate_ge", "no_dgamma", "per_chunk_n", "biased_running", "residual_after_act")
FWD_TRAIN = ("out", "save_mean", "save_rstd", "running_mean", "running_var")
BWD = ("dy", "dgamma", "dbeta", "dresidual")


def forward(y, gamma, beta, running_mean, running_var, nbt, eps, training, momentum, residual=None, act=0, slope=SLOPE,
            dtype=torch.float64, mutation=None):
    """-> dict(out, save_mean, save_rstd, running_mean, running_var, num_batches_tracked); the buffers passed in are not changed"""
    y, gamma, beta = y.to(dtype), gamma.to(dtype), beta.to(dtype)
    rm, rv = running_mean.to(dtype).clone(), running_var.to(dtype).clone()
    n = y.shape[0]
    if training:
        if n < 2:
            raise ValueError("Expected more than 1 value per channel when training")
        mean = y.sum(0) / n
        if mutation == "raw_moments":
            var = (y * y).sum(0) / n - mean * mean
        else:
            var = ((y - mean) ** 2).sum(0) / n
        norm_var = var * n / (n - 1) if mutation == "unbiased_norm" else var
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * (var if mutation == "biased_running" else var * n / (n - 1))
        nbt = nbt + 1
    else:
        mean, norm_var = rm.clone(), rv.clone()
    rstd = 1 / torch.sqrt(norm_var + eps)
    z = (y - mean) * rstd * gamma + beta
    if residual is not None and mutation != "residual_after_act":
        z = z + residual.to(dtype)
    out = torch.where(z > 0, z, z * slope) if act else z
    if residual is not None and mutation == "residual_after_act":
        out = out + residual.to(dtype)
    return {"out": out, "save_mean": mean, "save_rstd": rstd, "running_mean": rm, "running_var": rv, "num_batches_tracked": nbt}


def backward(dout, out_given, y, gamma, mean, rstd, training, act=0, slope=SLOPE, dtype=torch.float64, mutation=None):
    """-> dict(dy, dgamma, dbeta, dresidual); `out_given` decides the gate, element by element, whatever this dtype would
    have computed for it; mean / rstd are the forward's (save_mean / save_rstd, or the running statistics' in evaluation)"""
    dout, y, gamma, mean, rstd = (t.to(dtype) for t in (dout, y, gamma, mean, rstd))
    n = y.shape[0]
    if act:
        gate = (out_given >= 0) if mutation == "gate_ge" else (out_given > 0)
        dz = torch.where(gate, dout, dout * slope)
    else:
        dz = dout
    xhat = (y - mean) * rstd
    dbeta = dz.sum(0)
    dgamma = (dz * xhat).sum(0)
    if training:
        div = min(n, 256) if mutation == "per_chunk_n" else n
        second = 0 if mutation == "no_dgamma" else xhat * (dgamma / div)
        dy = gamma * rstd * (dz - dbeta / div - second)
    else:
        dy = gamma * rstd * dz
    return {"dy": dy, "dgamma": dgamma, "dbeta": dbeta, "dresidual": dz}


# ------------------------------------------------------------------------------------------------------------------
# the row table.  rows per chunk R, chunk count, merge depth and the column tile come from the plan of
# weasal_amd/csrc/batchnorm.hip (bn_plan): R = lanes * t with lanes = 256 / min(column groups, 64) and t = rows per thread,
# 1 until 256 workgroups exist and 8 at most; more than 1024 chunks raise R instead.  At c = 32 (vector path: 8 groups,
# 32 lanes) R is 32 below 16 384 rows; the merge depth is 0 for one chunk, 1 up to 64 chunks, 2 beyond.
# pad: (y, out, residual, dout, dy, dresidual) pitches above c; off: the tensor that starts one float off 16-byte alignment.
# ------------------------------------------------------------------------------------------------------------------
def _row(id, n, c, training=True, residual=False, act=False, momentum=0.02, data="normal", pad=0, off=None, dres=True):
    return dict(id=id, n=n, c=c, training=training, residual=residual, act=act, momentum=momentum, data=data, pad=pad, off=off,
                dres=dres and residual)


SHAPE_ROWS = (
    # N around the chunk length R = 32 of c = 32, the row lanes, the merge depths
    [_row("n%d-c32" % n, n, 32, act=True, residual=True) for n in (2, 3, 31, 32, 33, 63, 64, 65, 2048, 2049)]
    + [_row("n1-c32-eval", 1, 32, training=False, act=True, residual=True),
       _row("n16385-c32-two-rows-per-thread", 16385, 32, act=True),
       _row("n65539-c32-eight-rows-per-thread", 65539, 32, act=True, residual=True),
       _row("n700003-c3-chunk-cap", 700003, 3, act=True)]
    # every width class: scalar and vector column paths, a partly filled column tile, several column tiles
    + [_row("n257-c%d" % c, 257, c, act=True, residual=True) for c in (1, 3, 9, 16, 45, 64, 130, 256)]
    + [_row("n284-c1024", 284, 1024, act=True, residual=True), _row("n3-c1024-one-chunk-four-tiles", 3, 1024, act=True),
       _row("n2-c1", 2, 1), _row("n3-c4", 3, 4, act=True), _row("n63-c3", 63, 3, residual=True), _row("n777-c32", 777, 32, act=True),
       _row("n1031-c64", 1031, 64, act=True, residual=True), _row("n513-c130", 513, 130, act=True), _row("n2-c16", 2, 16, residual=True),
       _row("n4099-c130-depth2-scalar", 4099, 130, act=True, residual=True), _row("n300-c261-scalar-tiles", 300, 261, act=True),
       _row("n90001-c9-scalar-rows-per-thread", 90001, 9, act=True)]
)
MODE_ROWS = [_row("n257-c32-%s-res%d-act%d" % ("train" if t else "eval", r, a), 257, 32, training=t, residual=r, act=a)
             for t in (True, False) for r in (False, True) for a in (False, True)] + [
    _row("n257-c32-dres-null", 257, 32, residual=True, act=True, dres=False),
    _row("n257-c32-momentum-1", 257, 32, act=True, momentum=1.0),
    _row("n130-c9-eval-scalar", 130, 9, training=False, residual=True, act=True),
    # evaluation runs the apply kernel alone: its own walk of the column paths, tiles and rows per thread
    _row("n300-c261-eval-scalar-tiles", 300, 261, training=False, act=True),
    _row("n90001-c9-eval-scalar-rows-per-thread", 90001, 9, training=False, residual=True),
    _row("n700003-c3-eval-chunk-cap", 700003, 3, training=False, act=True),
    _row("n284-c1024-eval", 284, 1024, training=False, act=True, residual=True),
    _row("n16385-c32-eval-two-rows-per-thread", 16385, 32, training=False, act=True),
    _row("n33-c256-eval-full-tile", 33, 256, training=False, residual=True),
]
PITCH_ROWS = [_row("n65-c32-pitch-plus4", 65, 32, residual=True, act=True, pad=4),
              _row("n65-c32-pitch-plus1-scalar", 65, 32, residual=True, act=True, pad=1),
              _row("n65-c9-pitch-plus3", 65, 9, residual=True, act=True, pad=3)]
ALIGN_ROWS = [_row("n65-c32-off-%s" % name, 65, 32, residual=True, act=True, off=name)
              for name in ("y", "out", "residual", "dout", "dy", "dresidual")]
DATA_ROWS = [_row("n1031-c32-%s" % d, 1031, 32, residual=(d != "constcol"), act=True, data=d)
             for d in ("bigmean", "negmean", "tinystd", "constcol")] + [
    _row("n257-c9-bigmean-eval", 257, 9, training=False, act=True, data="bigmean"),
    _row("n5000-c16-bigmean", 5000, 16, act=True, data="bigmean"),
]
ROWS = SHAPE_ROWS + MODE_ROWS + PITCH_ROWS + ALIGN_ROWS + DATA_ROWS
BY_ID = {r["id"]: r for r in ROWS}
assert len(BY_ID) == len(ROWS)
CPU_ROWS = [r["id"] for r in ROWS if r["n"] * r["c"] <= 40000]      # the rows the CPU file's negative control walks


def inputs(row):
    """the float32 inputs of a row, from its own seed: y, gamma, beta, running_mean, running_var, residual | None, dout"""
    n, c = row["n"], row["c"]
    g = torch.Generator().manual_seed(sum(map(ord, row["id"])) * 7919 + n * 31 + c)
    y = torch.randn(n, c, generator=g)
    if row["data"] == "bigmean":          # |mean| / std = 1e3
        y = y + 1000.0
    elif row["data"] == "negmean":        # mean -300, std 5
        y = y * 5.0 - 300.0
    elif row["data"] == "tinystd":        # std 1e-3
        y = y * 1e-3 + 0.25
    elif row["data"] == "constcol":       # one column without variance: xhat = 0 there, out = beta = 0 exactly
        y[:, 2] = 2.0
    gamma = torch.rand(c, generator=g) + 0.5
    beta = torch.randn(c, generator=g) * 0.3
    if c >= 3:
        gamma[0], gamma[1] = 0.0, -1.3    # a zero and a negative scale
        beta[2] = 0.0
    rm = torch.randn(c, generator=g) * 0.5 + (1000.0 if row["data"] == "bigmean" else 0.0)
    rv = torch.rand(c, generator=g) + 0.5
    res = torch.randn(n, c, generator=g) if row["residual"] else None
    dout = torch.randn(n, c, generator=g)
    return y, gamma, beta, rm, rv, res, dout


def evaluate(row, dtype, given_out=None, mutation=None):
    """forward and backward of a row in `dtype`; the gate of the backward comes from `given_out` (default: this forward's)"""
    y, gamma, beta, rm, rv, res, dout = inputs(row)
    act = 1 if row["act"] else 0
    f = forward(y, gamma, beta, rm, rv, 0, EPS, row["training"], row["momentum"], res, act, SLOPE, dtype, mutation)
    out = f["out"] if given_out is None else given_out
    b = backward(dout, out, y, gamma, f["save_mean"], f["save_rstd"], row["training"], act, SLOPE, dtype, mutation)
    return {**f, **b}


@functools.lru_cache(maxsize=None)
def case(row_id):
    """(inputs, given_out float32, ref64, err32): the float32 restatement's output is THE `out` every backward gates by, so
    no comparison can see an activation-kink flip; err32[name] = max |float32 restatement - ref64|"""
    row = BY_ID[row_id]
    r32 = evaluate(row, torch.float32)
    given = r32["out"].clone()
    r64 = evaluate(row, torch.float64, given_out=given)
    names = tensors(row)
    err32 = {k: float((r32[k].double() - r64[k]).abs().max()) if r64[k].numel() else 0.0 for k in names}
    return inputs(row), given, {k: r64[k] for k in names + ("num_batches_tracked",)}, err32


def tensors(row):
    names = (FWD_TRAIN if row["training"] else ("out",)) + BWD
    return tuple(k for k in names if k != "dresidual" or row["residual"])


def violations(got, r64, err32, names=None):
    """{name: (error, bound)} of the tensors outside 4 * err32 + 1e-6 * max |ref64|; every element takes part"""
    bad = {}
    for k in names or err32:
        ref = r64[k]
        if not ref.numel():
            continue
        err = float((got[k].double().cpu() - ref).abs().max())
        bound = 4.0 * err32[k] + 1e-6 * float(ref.abs().max())
        if not err <= bound:
            bad[k] = (err, bound)
    return bad
