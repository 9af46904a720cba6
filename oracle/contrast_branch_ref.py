"""oracle/contrast_branch_ref.py -- TEST INFRASTRUCTURE ONLY (numpy, float64).

References of the eleven kernels of the supervised contrastive term (weasal_amd/csrc/contrast_mfma.hip, contrast_head.hip)
for tests/test_contrast_branches_*.py, one function per C entry, written from the contracts in include/weasal_hip.h and the
meaning of models/architectures.py:405-504 (dense masks, two passes: max, then sums), never from the kernels.  Every function
takes the float32 arrays the kernel takes (and its float arguments T / eps / threshold as the float32 values the kernel
receives, widened by the caller), computes in float64 and returns, next to each value, the per-element bound that
the float32 kernel is held to.

Error model (u = 2^-24; first order in u; never a fraction of a tensor's maximum).

  sums          k float32 terms added in any order whose longest chain has at most k + C additions:
                |got - ref| <= (k + C) u sum|terms|, k = the number of NON-ZERO terms (adding a zero is exact).  C per shape:
                  row statistics E, S     the 16-lane butterfly after the per-lane chains: 4 levels           C = 4
                  d_on                    the 4-wide matrix-core step inside the chain                        C = 4
                  d_xs                    4 (matrix-core step) + 2 (four-wave sum) + 5 (chunks in strides of
                                          32, then a 5-level tree)                                            C = 11
                  tail                    at most 16 rows per thread, an 8-level tree, then one addition per
                                          workgroup: a chain of min(k, 24 + workgroups) additions, + 2 for the
                                          two divisions
  similarities  mul_ij = <on_i, xs_j> / T: e_mul = ((c + 2) sum_ch |on xs| + 2 |<on, xs>|) u / T  (c products summed, the
                reciprocal of T and the product with it).  rowmax is a maximum of such values: e_m = max_j e_mul_ij.
  exponential   the fast exponential is exp2(a * log2(e)): the product rounds the exponent by |a| log2(e) u, which is a
                RELATIVE error |a| u of the result (twice: the constant is rounded too), plus the intrinsic's 1 ulp = 2 u.
                A term exp(mul - m) of den is the product of two of them (arguments a = mul - 1/T and b = 1/T - m, each in
                [-2/T, 0]; the rounding of 1/T cancels between them), each argument a rounded difference:
                  rel_ij = e_mul_ij + e_m + (3 |a| + 3 |b| + 5) u
  den           e_den = sum_j use_ij exp(mul_ij - m_i) rel_ij + (k + 4 + 1) u E + u den   (k usable columns; the product
                with the rebasing factor; the addition of eps)
  loss          num = (S - P m) - P log(den),  loss = -T num / (P + 1e-12):
                  e_num = sum_pos e_mul + (P + 4) u sum_pos |mul| + P e_m + u P |m| + u |S - P m|
                          + P (e_den / den + 2 u |log den|) + u P |log den| + u |num|
                  e_loss = T e_num / max(P, 1) + 3 u |loss|
  W             W_ij = gc_i (pos_ij - x_ij), x_ij = use_ij P_i exp(mul_ij - rowmax_i) / den_i, gc_i = -g_i / (P_i + 1e-12) (the
                backward takes rowmax / den / npos as INPUTS, so the reference uses the same float32 values):
                  e_W = |gc| x (e_mul + (3 |mul - rowmax| + 5) u) + 5 u |W|
                and through W:  e_d_on = e_W |xs| + (k_i + 4) u |W| |xs|,   e_d_xs = e_W^T |on| + (k_j + 11) u |W|^T |on|.
  head          on = x / max(|x|, 1e-12), inv_norm: c squares summed, a square root, a division: (c / 2 + 4) u relative.
  normalise^T   d_x = (g - on <g, on>) inv_norm (clamped rows: g inv_norm):
                  e = inv_norm (|on| (c + 2) u sum|g on| + 2 u (|g| + |on <g, on>|)) + 2 u |d_x|
No term of this model is set from a float32 restatement: all are derived above.

Compared exactly (no bound): npos, certain, lbl (outside the rows `head_ref` marks as undecidable in float32), slc_idx,
state, xs == on[slc_idx], the slice add (float32, slot order), g_row = g * w_cls[k], the class selection of the tail.
"""
import zlib

import numpy as np

U = 2.0 ** -24
C_BUTTERFLY, C_DON, C_DXS = 4.0, 4.0, 11.0
S_MAX = 1024                                   # slice rows every entry takes
T_MIN, T_MAX = 0.023, 1.0e26                   # temperatures the rows entries take (include/weasal_hip.h)

MUTATIONS = ("self", "certain", "max_usable", "pad", "eps_first", "xs_hi", "dup_last")
LAYOUT_MUTATIONS = ("pad", "xs_hi", "dup_last")    # must show on every instantiation they apply to


def f64(a):
    return np.asarray(a, np.float64)


# ------------------------------------------------------------------------------------------------------------------
# rows: ws_contrast_rows_fwd / _bwd
# ------------------------------------------------------------------------------------------------------------------
def _masks(n, slc_idx, certain, lbl):
    slc_idx = np.asarray(slc_idx, np.int64)
    certain = np.asarray(certain).astype(bool)
    lbl = np.asarray(lbl, np.int64)
    i = np.arange(n, dtype=np.int64)[:, None]
    use = (slc_idx[None, :] != i) & (certain[slc_idx][None, :] == certain[:, None])
    pos = use & (lbl[slc_idx][None, :] == lbl[:, None])
    return use, pos


def _similarities(on, xs, temperature):
    on, xs = f64(on), f64(xs)
    c = on.shape[1]
    t = float(temperature)
    d = on @ xs.T
    e_mul = ((c + 2) * (np.abs(on) @ np.abs(xs).T) + 2 * np.abs(d)) * U / t
    return d / t, e_mul, t


def rows_ref(on, xs, slc_idx, certain, lbl, temperature, eps, mutate=None):
    """dict(loss, rowmax, den, npos, b_loss, b_rowmax, b_den), float64 [n].  `mutate`: one of MUTATIONS -- a deliberately
    wrong reference (tests/test_contrast_branches_cpu.py shows that the bounds reject each)."""
    on, xs = f64(on), f64(xs)
    n, c = on.shape
    s = xs.shape[0]
    slc_idx = np.asarray(slc_idx, np.int64)
    if n == 0:
        z = np.zeros(0)
        return dict(loss=z, rowmax=z, den=z, npos=z, b_loss=z, b_rowmax=z, b_den=z)
    if mutate == "xs_hi":
        xs = xs.copy()
        xs[:, 12:16] = 0.0
    use, pos = _masks(n, slc_idx, certain, lbl)
    if mutate == "certain":
        use = slc_idx[None, :] != np.arange(n)[:, None]
        pos = use & (np.asarray(lbl)[slc_idx][None, :] == np.asarray(lbl)[:, None])
    if mutate == "self":
        vals, cnt = np.unique(slc_idx, return_counts=True)
        if (cnt > 1).any():
            q = int(vals[cnt > 1][0])
            slot = int(np.nonzero(slc_idx == q)[0][1])
            use[q, slot] = True
            pos[q, slot] = True
    if mutate == "pad" and s % 16:
        xs = np.concatenate([xs, np.zeros((1, c))], 0)
        use = np.concatenate([use, np.ones((n, 1), bool)], 1)
        pos = np.concatenate([pos, np.zeros((n, 1), bool)], 1)
    mul, e_mul, t = _similarities(on, xs, temperature)
    eps = float(eps)
    m = mul.max(1)
    if mutate == "max_usable":
        mu = np.where(use, mul, -np.inf).max(1)
        m = np.where(np.isfinite(mu), mu, m)
    e_m = e_mul.max(1)
    lg = mul - m[:, None]
    ex = np.exp(lg) * use
    E = ex.sum(1)
    den = E + eps
    if mutate == "eps_first":
        den = E + eps * np.exp(1.0 / t - m)
    k = use.sum(1).astype(np.float64)
    P = pos.sum(1).astype(np.float64)
    rel = e_mul + e_m[:, None] + (3 * np.abs(mul - 1.0 / t) + 3 * np.abs(1.0 / t - m)[:, None] + 5) * U
    e_den = (ex * rel).sum(1) + (k + C_BUTTERFLY + 1) * U * E + U * den
    Sp = (mul * pos).sum(1)
    logd = np.log(den)
    num = (Sp - P * m) - P * logd
    loss = -t * num / (P + 1e-12)
    e_num = (e_mul * pos).sum(1) + (P + C_BUTTERFLY) * U * (np.abs(mul) * pos).sum(1) + P * e_m + U * P * np.abs(m) \
        + U * np.abs(Sp - P * m) + P * (e_den / den + 2 * U * np.abs(logd)) + U * P * np.abs(logd) + U * np.abs(num)
    e_loss = t * e_num / np.maximum(P, 1.0) + 3 * U * np.abs(loss)
    out = dict(loss=loss, rowmax=m, den=den, npos=P, b_loss=e_loss, b_rowmax=e_m + U * np.abs(m), b_den=e_den)
    if mutate == "dup_last" and n % 16 and n >= 2:
        for key in ("loss", "rowmax", "den", "npos"):
            out[key] = out[key].copy()
            out[key][n - 1] = out[key][n - 2]
    return out


def rows_bwd_ref(on, xs, slc_idx, certain, lbl, temperature, eps, g, rowmax=None, den=None, npos=None):
    """dict(d_on [n,c], d_xs [s,c], b_d_on, b_d_xs): the gradients of sum_i g_i loss_i with the maximum detached.  The saved
    statistics rowmax / den / npos are the forward reference's, or the arrays given (what the backward entry is handed)"""
    on, xs = f64(on), f64(xs)
    if rowmax is None:
        fwd = rows_ref(on, xs, slc_idx, certain, lbl, temperature, eps)
        rowmax, den, npos = fwd["rowmax"], fwd["den"], fwd["npos"]
    n, c = on.shape
    s = xs.shape[0]
    if n == 0:
        return dict(d_on=np.zeros((0, c)), d_xs=np.zeros((s, c)), b_d_on=np.zeros((0, c)), b_d_xs=np.zeros((s, c)))
    use, pos = _masks(n, slc_idx, certain, lbl)
    mul, e_mul, _t = _similarities(on, xs, temperature)
    P = f64(npos)
    gc = -f64(g) / (P + 1e-12)
    lg = mul - f64(rowmax)[:, None]
    x = use * (P / f64(den))[:, None] * np.exp(lg)
    W = gc[:, None] * (pos - x)
    e_W = np.abs(gc)[:, None] * x * (e_mul + (3 * np.abs(lg) + 5) * U) + 5 * U * np.abs(W)
    ki = use.sum(1).astype(np.float64)[:, None]
    kj = use.sum(0).astype(np.float64)[:, None]
    aW = np.abs(W)
    return dict(d_on=W @ xs, d_xs=W.T @ on,
                b_d_on=e_W @ np.abs(xs) + (ki + C_DON) * U * (aW @ np.abs(xs)),
                b_d_xs=e_W.T @ np.abs(on) + (kj + C_DXS) * U * (aW.T @ np.abs(on)))


# ------------------------------------------------------------------------------------------------------------------
# head: ws_contrast_head_fwd
# ------------------------------------------------------------------------------------------------------------------
def head_ref(x, labels, threshold):
    """dict(maxp, arg, certain, lbl, on, inv_norm, b_on, b_inv_norm, undecided): undecided [n] bool marks the unlabelled rows
    whose certain / lbl float32 cannot decide: the max-probability within 1e-5 of the threshold, or the top two
    probabilities within 1e-5 relative of each other"""
    x = f64(x)
    n, c = x.shape
    labels = np.asarray(labels, np.int64)
    thr = float(threshold)
    e = np.exp(x - x.max(1, keepdims=True))
    prob = e / e.sum(1, keepdims=True)
    arg = prob.argmax(1)                                      # the first maximum
    maxp = prob.max(1)
    labelled = labels < 10
    certain = (maxp > thr) | labelled
    lbl = np.where(labelled, labels, arg)
    if c > 1:
        top2 = np.sort(prob, 1)[:, -2:]
        tie = (top2[:, 1] - top2[:, 0]) <= 1e-5 * top2[:, 1]
    else:
        tie = np.zeros(n, bool)
    undecided = ~labelled & ((np.abs(maxp - thr) <= 1e-5) | tie)
    nrm = np.sqrt((x * x).sum(1))
    inv = 1.0 / np.maximum(nrm, 1e-12)
    on = x * inv[:, None]
    rel = (c / 2.0 + 4.0) * U
    return dict(maxp=maxp, arg=arg, certain=certain, lbl=lbl, on=on, inv_norm=inv, b_on=rel * np.abs(on), b_inv_norm=rel * inv,
                undecided=undecided)


def select_ref(certain, draw, s, n=None):
    """(slc_idx [s] int64, num_valid).  draw: int64 positions r [s] in the list of valid points, or float32 uniforms u [s]:
    r_j = floor(u_j * num_valid) as a float32 product, and with fewer valid points than slots, slot j < num_valid takes
    valid point j.  r is clamped to [0, num_valid - 1]; no valid point: n - 1 everywhere."""
    certain = np.asarray(certain).astype(bool)
    n = certain.shape[0] if n is None else n
    valid = np.nonzero(certain)[0].astype(np.int64)
    nv = valid.shape[0]
    draw = np.asarray(draw)
    if nv == 0:
        return np.full(s, n - 1, np.int64), 0
    if draw.dtype == np.float32:
        r = np.floor(draw * np.float32(nv)).astype(np.int64)
        j = np.arange(s)
        if nv < s:
            r = np.where(j < nv, j, r)
    else:
        r = draw.astype(np.int64)
    return valid[np.clip(r, 0, nv - 1)], nv


# ------------------------------------------------------------------------------------------------------------------
# tail: ws_contrast_tail_fwd / _bwd
# ------------------------------------------------------------------------------------------------------------------
def tail_ref(pts_loss, lbl, n_cls, num_valid):
    """dict(per_class, w_cls, loss, b_per_class, b_w_cls, b_loss, sel); labels outside [0, n_cls) fall into the nearest bin"""
    v = f64(pts_loss)
    n = v.shape[0]
    k = np.clip(np.asarray(lbl, np.int64), 0, n_cls - 1)
    keep = v > 0
    sums = np.bincount(k[keep], weights=v[keep], minlength=n_cls)
    cnt = np.bincount(k[keep], minlength=n_cls).astype(np.float64)
    cn = np.maximum(cnt, 1.0)
    per_class = sums / cn
    sel = per_class > 0
    nsel = float(sel.sum())
    nblk = -(-n // 4096)
    e_pc = (np.minimum(cnt, 24.0 + nblk) + 2) * U * per_class
    with np.errstate(invalid="ignore", divide="ignore"):
        if num_valid <= 0:
            loss, w = 0.0, np.zeros(n_cls)
            e_loss = 0.0
        else:
            loss = (per_class * sel).sum() / nsel
            w = sel / (nsel * cn)
            e_loss = (e_pc * sel).sum() / nsel + (n_cls + 2) * U * abs(loss)
    return dict(per_class=per_class, w_cls=w, loss=loss, b_per_class=e_pc, b_w_cls=2 * U * np.abs(w), b_loss=e_loss, sel=sel)


def tail_bwd_ref(pts_loss, lbl, n_cls, w_cls, g):
    """g_row [n] float32 = g * w_cls[bin] where pts_loss > 0, else 0: one float32 product, exact"""
    v = np.asarray(pts_loss, np.float32)
    k = np.clip(np.asarray(lbl, np.int64), 0, n_cls - 1)
    w = np.asarray(w_cls, np.float32)
    return np.where(v > 0, np.float32(g) * w[k], np.float32(0)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------
# head backward: slice add, backward of the normalisation
# ------------------------------------------------------------------------------------------------------------------
def slice_add_ref(d_on, d_xs, slc_idx):
    """d_on with the slice rows' gradients added onto their points, in d_on's dtype: a point's slots are added in slot order
    onto its row, ((d_on[p] + d_xs[j1]) + d_xs[j2]) + ... (the kernel states this order: float32 results are bit-equal)"""
    out = np.array(d_on, copy=True)
    d_xs = np.asarray(d_xs, out.dtype)
    for j, p in enumerate(np.asarray(slc_idx, np.int64)):
        out[p] = out[p] + d_xs[j]
    return out


def normalize_bwd_ref(d_on, on, inv_norm):
    """(d_x, bound): rows whose inv_norm is the clamp's 1e12 (|x| <= 1e-12) pass g * inv_norm, the others the projection"""
    g, o, inv = f64(d_on), f64(on), f64(inv_norm)
    c = g.shape[1]
    dot = (g * o).sum(1, keepdims=True)
    clamped = (inv >= 1e12 * (1 - 8 * U))[:, None]
    d_x = np.where(clamped, g, g - o * dot) * inv[:, None]
    sabs = (np.abs(g) * np.abs(o)).sum(1, keepdims=True)
    b = inv[:, None] * (np.abs(o) * (c + 2) * U * sabs + 2 * U * (np.abs(g) + np.abs(o * dot))) + 2 * U * np.abs(d_x)
    return d_x, b


def composed_loss_ref(x, labels, threshold, r_draw, temperature=0.1, eps=1e-8, n_cls=None, g=1.0):
    """the whole loss and its logits gradient from the references above, float64 throughout (r_draw: int64 positions [s])"""
    x = f64(x)
    n, c = x.shape
    n_cls = max(c, 10) if n_cls is None else n_cls
    h = head_ref(x, labels, threshold)
    s = len(r_draw)
    slc, nv = select_ref(h["certain"], np.asarray(r_draw, np.int64), s, n)
    xs = h["on"][slc]
    r = rows_ref(h["on"], xs, slc, h["certain"], h["lbl"], temperature, eps)
    t = tail_ref(r["loss"], h["lbl"], n_cls, nv)
    k = np.clip(h["lbl"], 0, n_cls - 1)
    g_row = np.where(r["loss"] > 0, g * t["w_cls"][k], 0.0)
    b = rows_bwd_ref(h["on"], xs, slc, h["certain"], h["lbl"], temperature, eps, g_row)
    d_on = slice_add_ref(b["d_on"], b["d_xs"], slc)
    d_x, _ = normalize_bwd_ref(d_on, h["on"], h["inv_norm"])
    return dict(loss=t["loss"], d_x=d_x, num_valid=nv, slc_idx=slc, per_class=t["per_class"])


# ------------------------------------------------------------------------------------------------------------------
# launch plans (what the case tables must reach) and the case tables
# ------------------------------------------------------------------------------------------------------------------
def rows_plan(c, n, s):
    """the launch branches of ws_contrast_rows_fwd / _bwd at a shape, by name"""
    chunks = max(-(-n // 256), 1)
    return {"NS%d" % ((c + 3) // 4), "c%4=" + str(c % 4), "tile_partial" if n % 16 else "tile_full",
            "s_lt16" if s < 16 else ("s_padded" if s % 16 else "s_tiles"),
            "partial_is_d_xs" if chunks == 1 else ("reduce_1trip" if chunks <= 32 else "reduce_2trips"),
            "partial_is_d_xs_c%s9" % ("=" if c == 9 else "!") if chunks == 1 else "scratch"}


def head_plan(n, s):
    rpb = 256
    while -(-n // rpb) > 8192:
        rpb *= 2
    return {"rpb%d" % rpb, "blocks1" if n <= rpb else "blocks_many", "select_grid%d" % min(-(-s // 64), 3)}


def tail_plan(n):
    nblk = -(-n // 4096)
    return {"tail_blocks1" if nblk == 1 else "tail_blocks_many", "stage_passes%d" % (-(-nblk // 128))}


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# (id, c, n, s, T, pattern): the C / s / n ladders, the corners and the temperatures, on the "mixed" data; then the data patterns
ROWS_CASES = []
for _c in (1, 4, 5, 8, 9, 12, 13, 16):
    ROWS_CASES.append(("c%d" % _c, _c, 257, 1000, 0.1, "mixed"))
for _s in (1, 15, 16, 17, 1000, 1024):
    ROWS_CASES.append(("s%d" % _s, 9, 300, _s, 0.1, "mixed"))
for _n in (1, 16, 17, 255, 256, 257, 8192, 8193):
    ROWS_CASES.append(("n%d" % _n, 9, _n, 1000, 0.1, "mixed"))
ROWS_CASES += [("corner_min", 1, 1, 1, 0.1, "mixed"), ("corner_max", 16, 8193, 1024, 0.1, "mixed")]
for _t in (0.05, 1.0):
    ROWS_CASES.append(("T%g" % _t, 9, 300, 1000, _t, "mixed"))
for _p, _c, _n, _s in (("valid_slice", 9, 300, 1000), ("one_label", 4, 257, 1000), ("repeat", 13, 257, 1000),
                       ("repeat", 5, 100, 37), ("one_point", 1, 257, 1000), ("one_point", 9, 40, 17),
                       ("one_point", 16, 257, 1000), ("mixed", 4, 100, 1000), ("mixed", 16, 100, 40), ("mixed", 5, 256, 999),
                       ("mixed", 13, 17, 1001)):
    ROWS_CASES.append(("%s_c%d_n%d_s%d" % (_p, _c, _n, _s), _c, _n, _s, 0.1, _p))

ROWS_PATTERNS = ("mixed", "valid_slice", "one_label", "repeat", "one_point")


def make_rows_case(c, n, s, pattern, key=0):
    """float32 / int64 / uint8 numpy inputs of the rows entries.  Patterns (n >= 8 for the marked rows):
      mixed        70 % certain points, labels in [0, min(c, 16)) (up to 15 at C = 16), the slice drawn from ALL points;
                   row 0 all-zero, row 1 = +e_0, row 2 = -e_(c-1) (a component exactly +-1), point 3 with given label 9
                   (at every C, C = 4 included), point 4 with a label no slice point has (P = 0), kept out of the slice
      valid_slice  as mixed, the slice from the certain points only: no uncertain point has a usable column (E = 0)
      one_label    every point certain, one label
      repeat       point 6 in the slots {0, 15, 16, 17, 31, 32, 33, s - 1} (across the 16-column tiles; row 6 meets itself)
      one_point    the slice is point 5, s times; at C = 1 the rows are +-1
    g: zeros (10 %), both signs, magnitudes over six decades."""
    rng = _rng("rows", c, n, s, pattern, key)
    raw = rng.standard_normal((n, c))
    raw = np.where(np.abs(raw) < 1e-3, 1e-3, raw)
    on = (raw / np.sqrt((raw * raw).sum(1, keepdims=True))).astype(np.float32)
    certain = rng.random(n) < 0.7
    lbl = rng.integers(0, max(min(c, 16), 2), size=n).astype(np.int64)
    special = n >= 8
    if pattern == "one_label":
        certain[:] = True
        lbl[:] = 3
    if special and pattern != "one_label":
        on[0] = 0.0
        on[1] = 0.0
        on[1, 0] = 1.0
        on[2] = 0.0
        on[2, c - 1] = -1.0
        lbl[3] = 9
        lbl[4] = 31
    pool = np.arange(n)
    if special:
        pool = pool[pool != 4]
    if pattern == "valid_slice":
        certain[5] = True
        pool = pool[certain[pool]]
    slc = pool[rng.integers(0, pool.size, size=s)].astype(np.int64)
    if pattern == "repeat" and special:
        for j in (0, 15, 16, 17, 31, 32, 33, s - 1):
            if 0 <= j < s:
                slc[j] = 6
    if pattern == "one_point":
        slc[:] = min(5, n - 1)
    g = (10.0 ** rng.uniform(-3, 3, size=n) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)
    g[rng.random(n) < 0.1] = 0.0
    return dict(on=on, xs=on[slc].copy(), slc_idx=slc, certain=certain.astype(np.uint8), lbl=lbl, g=g)


# head: (id, c, n, s, pad (ldx - c), threshold, scale, valid): `valid` shapes where the valid points lie
HEAD_CASES = [("c1", 1, 257, 64, 0, 0.3, 1.5, "spread"), ("c2", 2, 257, 65, 0, 0.6, 1.5, "spread"),
              ("c9", 9, 70001, 1000, 0, 0.4, 1.5, "spread"), ("c10", 10, 257, 63, 3, 0.3, 1.5, "spread"),
              ("c15", 15, 255, 1, 0, 0.2, 1.5, "spread"), ("c16", 16, 256, S_MAX, 4, 0.2, 1.5, "spread"),
              ("n1", 9, 1, 1000, 0, 0.2, 1.5, "spread"), ("n1_none", 9, 1, 5, 0, 0.99, 0.01, "none"),
              ("near_uniform", 9, 2000, 1000, 0, 0.2, 0.01, "spread"),
              ("first_block", 9, 70001, 1000, 0, 0.99, 0.01, "first"), ("last_block", 9, 70001, 1000, 0, 0.99, 0.01, "last"),
              ("runs", 9, 70001, 1000, 7, 0.99, 0.01, "runs"), ("none", 9, 1000, 64, 0, 0.99, 0.01, "none"),
              ("one", 9, 1000, 64, 0, 0.99, 0.01, "one"), ("nv_s-1", 9, 1000, 64, 0, 0.99, 0.01, 63),
              ("nv_s", 9, 1000, 64, 0, 0.99, 0.01, 64), ("nv_s+1", 9, 1000, 64, 0, 0.99, 0.01, 65),
              ("all", 9, 1000, 64, 0, 0.05, 1.5, "spread"),
              ("rpb256_top", 2, 2097152, 1000, 0, 0.6, 1.5, "spread"), ("rpb512", 2, 2097153, 1000, 0, 0.6, 1.5, "spread")]


def make_head_case(c, n, s, pad, scale, valid, key=0):
    """x [n, c + pad] float32 (the kernel takes the first c columns: ldx > c), labels [n] int64 with the values {0, 9, 10,
    100, -1}: < 10 = given (certain whatever the logits say; -1 included), the rest unlabelled.  `valid`: "spread" = 2 % of
    the points given at random; "none"; "one"; "first" / "last" = only in the first / last 256 rows; "runs" = a few given
    points every 20 000 rows (runs of empty blocks between); an int = that many given points.  Row 7 is all-zero (n > 7)."""
    rng = _rng("head", c, n, s, pad, scale, valid, key)
    x = (rng.standard_normal((n, c + pad)) * scale).astype(np.float32)
    labels = np.where(rng.random(n) < 0.5, 10, 100).astype(np.int64)
    if valid == "spread":
        given = np.nonzero(rng.random(n) < 0.02)[0]
    elif valid == "none":
        given = np.zeros(0, np.int64)
    elif valid == "one":
        given = np.array([n // 2])
    elif valid == "first":
        given = np.arange(3, min(n, 256), 5)
    elif valid == "last":
        given = np.arange(max(n - 200, 0), n, 3)
    elif valid == "runs":
        given = np.concatenate([np.arange(b, min(b + 3, n)) for b in range(100, n, 20000)])
    else:
        given = rng.permutation(n)[:int(valid)]
    labels[given] = rng.choice([0, 9, -1], size=given.size)
    if n > 7:
        x[7] = 0.0
    return x, labels


TAIL_CASES = [(n, k) for n in (1, 4095, 4096, 4097) for k in (1, 10, 16)] + [(524288, 10), (524289, 16)]


def make_tail_case(n, n_cls, key=0):
    """pts_loss [n] float32 (a third <= 0, zeros included), lbl [n] int64 in [-2, n_cls + 2) (outside the bins at both ends);
    n_cls >= 10: bin 4 empty, every loss of bin 6 <= 0"""
    rng = _rng("tail", n, n_cls, key)
    v = rng.uniform(-0.5, 1.0, size=n).astype(np.float32)
    v[rng.random(n) < 0.05] = 0.0
    lbl = rng.integers(-2, n_cls + 2, size=n).astype(np.int64)
    if n_cls >= 10:
        lbl[lbl == 4] = 5
        v[lbl == 6] = -np.abs(v[lbl == 6])
    return v, lbl


# head backward: (c, n, s, pad (ldd - c), pattern)
HEAD_BWD_CASES = [(9, 300, 1, 0, "dups"), (1, 300, 4, 0, "dups"), (16, 300, 5, 0, "dups"), (9, 300, 64, 3, "dups"),
                  (9, 300, 65, 0, "dups"), (9, 300, 1000, 0, "dups"), (16, 2000, S_MAX, 5, "dups"), (9, 300, 1000, 0, "same"),
                  (1, 5, 65, 0, "same"), (9, 70001, 1000, 0, "random")]


def make_head_bwd_case(c, n, s, pattern, key=0):
    """d_on [n,c], d_xs [s,c], slc_idx [s], on [n,c], inv_norm [n] (float32 / int64).  "dups": point 3 in the slots {j, j + 1,
    63, 64, 65, s - 1} (j = 1), point 4 in two far slots; "same": every slot the same point; rows 0 and 1 clamped
    (inv_norm = the float32 1 / 1e-12f: a zero row and a row of norm 1e-13)."""
    rng = _rng("head_bwd", c, n, s, pattern, key)
    x = rng.standard_normal((n, c)).astype(np.float32)
    x[0] = 0.0
    if n > 1:
        x[1] = 0.0
        x[1, 0] = 1e-13
    nrm = np.sqrt((x.astype(np.float64) ** 2).sum(1))
    one = np.float32(1.0)
    inv = (one / np.maximum(nrm.astype(np.float32), np.float32(1e-12))).astype(np.float32)
    on = (x / np.maximum(nrm.astype(np.float32), np.float32(1e-12))[:, None]).astype(np.float32)
    slc = rng.integers(0, n, size=s).astype(np.int64)
    if pattern == "dups":
        for j in (1, 2, 63, 64, 65, s - 1):
            if 0 <= j < s:
                slc[j] = min(3, n - 1)
        for j in (0, s // 2):
            slc[j] = min(4, n - 1) if s > 8 else slc[j]
    if pattern == "same":
        slc[:] = min(1, n - 1)
    d_on = (rng.standard_normal((n, c)) * 10.0 ** rng.uniform(-3, 3, size=(n, 1))).astype(np.float32)
    d_xs = (rng.standard_normal((s, c)) * 10.0 ** rng.uniform(-3, 3, size=(s, 1))).astype(np.float32)
    return dict(d_on=d_on, d_xs=d_xs, slc_idx=slc, on=on, inv_norm=inv)
