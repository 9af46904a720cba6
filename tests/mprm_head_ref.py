"""Float64 restatements of what follows the attention blocks in the weak-label step, written out as formulas (no autograd,
nothing from the device library): the per-sphere mean, the maximum over heads with the tie rule of torch's maximum, the
multi-head BCE with logits, and clip-by-norm followed by the SGD update.  tests/test_mprm_head_cpu.py pins each of them to
what the reference project itself calls (split / mean / stack, nested torch.max under autograd, BCEWithLogitsLoss(weight),
clip_grad_norm_ + torch.optim.SGD) in float64; tests/test_mprm_head_gpu.py holds the kernels to them.

The `*_torch` functions are those calls themselves at a chosen dtype: in float32 they are the arithmetic the kernels replace,
the yardstick of the GPU tests' bound.
"""
import numpy as np
import torch

F64 = torch.float64


def spans(lengths):
    out, s = [], 0
    for n in lengths:
        out.append((s, s + int(n)))
        s += int(n)
    return out


# ---- per-sphere mean (models/blocks.py:114-134) ------------------------------------------------------------------------
def segment_mean(x, lengths):
    """out [B, W]: row sums divided by the length; an empty sphere is 0 / 0 = nan"""
    x = x.to(F64)
    out = torch.empty((len(lengths), x.shape[1]), dtype=F64)
    for b, (s, e) in enumerate(spans(lengths)):
        out[b] = x[s:e].sum(dim=0) / float(e - s) if e > s else float("nan")
    return out


def segment_mean_bwd(d_out, lengths):
    """dx [N, W]: dx[row] = d_out[sphere(row)] / length"""
    d_out = d_out.to(F64)
    rows = [d_out[b:b + 1].expand(e - s, -1) / float(e - s) for b, (s, e) in enumerate(spans(lengths)) if e > s]
    return torch.cat(rows, 0) if rows else d_out.new_zeros((0, d_out.shape[1]))


def segment_mean_torch(x, lengths, d_out, dtype):
    """the reference's loop at `dtype` with autograd -> (out, dx)"""
    x = x.to(dtype).clone().requires_grad_(True)
    out = torch.stack([chunk.mean(dim=0) for chunk in torch.split(x, [int(v) for v in lengths], dim=0)])
    out.backward(d_out.to(dtype))
    return out.detach(), x.grad


# ---- maximum over heads (models/architectures.py:700-702) --------------------------------------------------------------
def max_heads(x, heads):
    c = x.shape[1] // heads
    m = x[:, :c]
    for k in range(1, heads):
        m = torch.where(x[:, k * c:(k + 1) * c] > m, x[:, k * c:(k + 1) * c], m)
    return m


def max_heads_bwd(x, heads, d_out):
    """the gradient of the nested maximum: per maximum(a, b) both sides start from (a == b ? g / 2 : g), a's is zero where
    a < b, b's where a > b; outermost first"""
    c = x.shape[1] // heads
    h = [x[:, k * c:(k + 1) * c] for k in range(heads)]
    m = [h[0]]
    for k in range(1, heads):
        m.append(torch.where(h[k] > m[-1], h[k], m[-1]))
    g = d_out.clone()
    parts = [None] * heads
    for k in range(heads - 1, 0, -1):
        a, b = m[k - 1], h[k]
        both = torch.where(a == b, g / 2, g)
        parts[k] = torch.where(a > b, torch.zeros_like(g), both)
        g = torch.where(a < b, torch.zeros_like(g), both)
    parts[0] = g
    return torch.cat(parts, dim=1)


def max_heads_torch(x, heads, d_out):
    """the nested torch.max under autograd -> (out, dx)"""
    x = x.clone().requires_grad_(True)
    c = x.shape[1] // heads
    m = x[:, :c]
    for k in range(1, heads):
        m = torch.max(m, x[:, k * c:(k + 1) * c])
    m.backward(d_out)
    return m.detach(), x.grad


# ---- multi-head BCE with logits (models/architectures.py:709-733, 778-783) ----------------------------------------------
def bce_heads(x, target, weight, heads):
    """-> (per_head [heads], total): mean over rows and columns of w[c] (max(x, 0) - x y + log1p(exp(-|x|)))"""
    x, y = x.to(F64), target.to(F64)
    c = y.shape[1]
    w = torch.ones(c, dtype=F64) if weight is None else weight.to(F64)
    per = []
    for k in range(heads):
        xk = x[:, k * c:(k + 1) * c]
        per.append((w * (xk.clamp(min=0) - xk * y + torch.log1p(torch.exp(-xk.abs())))).sum() / float(y.numel()))
    per = torch.stack(per)
    return per, per.sum()


def bce_heads_bwd(x, target, weight, heads, g_heads, g_sum):
    """dx [R, heads C] = (g_heads[k] + g_sum) w[c] (sigmoid(x) - y) / (R C)"""
    x, y = x.to(F64), target.to(F64)
    c = y.shape[1]
    w = torch.ones(c, dtype=F64) if weight is None else weight.to(F64)
    e = torch.exp(-x.abs())
    sig = torch.where(x >= 0, 1 / (1 + e), e / (1 + e))
    g = (g_heads.to(F64) + float(g_sum)).repeat_interleave(c)
    return (sig - y.repeat(1, heads)) * w.repeat(heads) * g / float(y.numel())


def bce_heads_torch(x, target, weight, heads, g_heads, g_sum, dtype):
    """BCEWithLogitsLoss(weight) per column block at `dtype`, with autograd -> (per_head, total, dx)"""
    x = x.to(dtype).clone().requires_grad_(True)
    y = target.to(dtype)
    c = y.shape[1]
    crit = torch.nn.BCEWithLogitsLoss(weight=None if weight is None else weight.to(dtype))
    per = [crit(x[:, k * c:(k + 1) * c], y) for k in range(heads)]
    total = per[0]
    for p in per[1:]:
        total = total + p
    ((torch.stack(per) * g_heads.to(dtype)).sum() + total * float(g_sum)).backward()
    return torch.stack(per).detach(), total.detach(), x.grad


# ---- clip by norm, then SGD (utils/trainer_WeakLabel.py:216 and the optimizer step) --------------------------------------
def clip_sgd(params, grads, bufs, lr, momentum, weight_decay, max_norm):
    """one step on float64 copies -> (params, bufs, grads as clipped, total_norm); bufs: None on the first step"""
    p64 = [p.to(F64) for p in params]
    g64 = [g.to(F64) for g in grads]
    total = float(np.sqrt(sum(float((g * g).sum()) for g in g64)))
    coef = min(1.0, max_norm / (total + 1e-6))
    out_p, out_b, out_g = [], [], []
    for i, (p, g) in enumerate(zip(p64, g64)):
        g = g * coef
        out_g.append(g)
        d = g + weight_decay * p if weight_decay != 0 else g
        if momentum != 0:
            d = d if bufs is None else momentum * bufs[i].to(F64) + d
            out_b.append(d)
        out_p.append(p - lr * d)
    return out_p, out_b, out_g, total


def clip_sgd_torch(params, grads, steps, lr, momentum, weight_decay, max_norm, dtype):
    """clip_grad_norm_ + torch.optim.SGD at `dtype`, `steps` steps with the same gradients each
    -> (params, momentum buffers or [], p.grad after the last step, total_norm of the last step)"""
    ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in params]
    opt = torch.optim.SGD(ps, lr=lr, momentum=momentum, weight_decay=weight_decay)
    for _ in range(steps):
        for p, g in zip(ps, grads):
            p.grad = g.to(dtype).clone()
        norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
    bufs = [opt.state[p]["momentum_buffer"].detach() for p in ps] if momentum != 0 else []
    return [p.detach() for p in ps], bufs, [p.grad for p in ps], norm.detach()
