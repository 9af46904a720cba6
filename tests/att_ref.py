"""Restatement of the three per-sphere attention forms of KPFCNN_mprm (models/blocks.py:758-1011) and their gradients, in
plain torch with autograd, in the dtype of its inputs: float64 is the reference of the attention tests, float32 on the CPU
is the arithmetic of the module loops (the yardstick the kernels' error is measured against).

    spatial   att = softmax(Q K^T) V per sphere (no 1/sqrt(d) scale), xn = att / n_sphere
    channel   E = X1^T X2 per sphere, A = softmax_rows(rowmax(E) - E)  (channel_att)  or  softmax_rows(E)  (ele_att),
              out = Val A
"""
import torch


def spans(lengths):
    out, s = [], 0
    for n in lengths:
        out.append((s, s + int(n)))
        s += int(n)
    return out


def spatial(q, k, v, lengths):
    outs, outs_n = [], []
    for a, b in spans(lengths):
        att = torch.matmul(torch.softmax(torch.matmul(q[a:b], k[a:b].T), dim=-1), v[a:b])
        outs.append(att)
        outs_n.append(att / float(b - a))
    return torch.cat(outs, 0), torch.cat(outs_n, 0)


def channel(x1, x2, value, lengths, max_minus):
    outs = []
    for a, b in spans(lengths):
        energy = torch.matmul(x1[a:b].T, x2[a:b])
        if max_minus:
            energy = torch.max(energy, -1, keepdim=True)[0].expand_as(energy) - energy
        outs.append(torch.matmul(value[a:b], torch.softmax(energy, dim=-1)))
    return torch.cat(outs, 0)


def _leaves(tensors, dtype):
    return [t.detach().to("cpu", dtype).clone().requires_grad_(True) for t in tensors]


def spatial_with_grads(q, k, v, lengths, g_att, g_xn, dtype=torch.float64):
    """{att, xn, dq, dk, dv} on the CPU in `dtype` for the loss <att, g_att> + <xn, g_xn>"""
    ql, kl, vl = _leaves((q, k, v), dtype)
    att, xn = spatial(ql, kl, vl, lengths)
    loss = (att * g_att.to("cpu", dtype)).sum() + (xn * g_xn.to("cpu", dtype)).sum()
    dq, dk, dv = torch.autograd.grad(loss, (ql, kl, vl))
    return {"att": att.detach(), "xn": xn.detach(), "dq": dq, "dk": dk, "dv": dv}


def channel_with_grads(x1, x2, value, lengths, max_minus, g_out, dtype=torch.float64):
    """{out, dx1, dx2, dvalue} on the CPU in `dtype` for the loss <out, g_out>"""
    a, b, c = _leaves((x1, x2, value), dtype)
    out = channel(a, b, c, lengths, max_minus)
    loss = (out * g_out.to("cpu", dtype)).sum()
    d1, d2, dv = torch.autograd.grad(loss, (a, b, c))
    return {"out": out.detach(), "dx1": d1, "dx2": d2, "dvalue": dv}
