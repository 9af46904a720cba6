// weasal_amd/csrc/blocks.hip -- whole network blocks behind one C call (host code: launch sequences over the kernels
// of kpconv.hip / gemm.hip / pools.hip on one stream).
//
// Reference units: models/blocks.py:510-564 (SimpleBlock), :624-709 (ResnetBottleneckBlock) and their autograd;
// models/architectures.py:339-343 + blocks.py:473-507 (nearest_upsample -> concat -> unary).  The reference runs each
// of them as ~10 torch ops plus autograd nodes driven from Python; here one call launches the 6-7 (forward) or 10-14
// (backward) kernels back to back, every gradient accumulation is the residual operand of a GEMM epilogue and the
// scratch comes from one caller-owned arena (no allocation, no host synchronisation).
#include <vector>

#include "ws_common.h"

// diagnostics switch (WEASAL_BLOCK_GATES=0): activation backward as separate passes instead of epilogue / store gates
extern "C" int ws_block_gates = 1;
extern "C" int ws_block_gather_residual = 1;   // decoder step: 1 = the upsampled rows are gathered by the last epilogue, 0 = written out first (A/B)
// A/B switch (WEASAL_BLOCK_GROUP_ROWS=<rows>): blocks / decoder steps with fewer rows than this issue their mutually independent
// dense products as grouped launches (ws_priv_gemm_xb_group / ws_priv_gemm_xty_group): the weight-gradient products -- leaves
// of the backward, nothing waits for them -- are collected and launched at the end of the call, the two products that read
// dz ride together, and so do the two that read a block's input.  Every member keeps the plan it gets alone: results are
// bit-identical, only the launch count changes.  0 = off: the single launches in their old order.  The limit exists for the
// tall levels: deferring a leaf product there moves its read of a 205 MB gradient behind the KPConv backward's stream.
// Measured on the DALES step it does not hurt -- 12.55 ms with a limit of 32 768 or 80 000 rows, 12.47 without one, 12.69
// with the switch at 0 -- so the default is no limit.
extern "C" int64_t ws_block_group_rows = (int64_t)1 << 62;
// A/B switch (WEASAL_FUSED_INFER=0): forward-only blocks run gather + contraction as two launches like the training path
extern "C" int ws_block_fused_infer = 1;
// A/B switch (WEASAL_POOL_ORDER=0): the strided blocks' max-pool walks its rows by index instead of in cell order
extern "C" int ws_block_pool_order = 1;
// A/B switch (WEASAL_BLOCK_PACKED_K4=0): the table-walk K4 of a block through ws_kpconv_gather_bwd_x_gated instead of the packed entry
extern "C" int ws_block_packed_k4 = 1;

namespace {

struct Arena {
    char* base;
    int64_t cap, off;
    Arena(void* b, int64_t c) : base((char*)b), cap(c), off(0) {}
    template <typename T> T* take(int64_t count)
    {
        off = (off + 255) & ~(int64_t)255;
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += count * (int64_t)sizeof(T);
        return p;
    }
    bool fits() const { return off <= cap; }
};

// what the size queries report and the runs require: the plan, rounded up to the arena's 256-byte step, plus one step
inline int64_t arena_bytes(const Arena& ar) { return ((ar.off + 255) & ~(int64_t)255) + 256; }

inline int64_t max3(int64_t a, int64_t b, int64_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

__global__ __launch_bounds__(256) void transpose_small_kernel(const float* __restrict__ w, int rows, int cols, int64_t ld,
                                                               float* __restrict__ out)
{
    // out[c][r] = w[r*ld + c]   (weights: a few hundred KB at most)
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)rows * cols) return;
    const int c = (int)(e / rows), r = (int)(e % rows);
    out[e] = w[(int64_t)r * ld + c];
}

__global__ __launch_bounds__(256) void add_rows_kernel(float* __restrict__ a, const float* __restrict__ b, int64_t n4)
{
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n4; e += (int64_t)gridDim.x * 256) {
        float4 x = reinterpret_cast<float4*>(a)[e];
        const float4 y = reinterpret_cast<const float4*>(b)[e];
        x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
        reinterpret_cast<float4*>(a)[e] = x;
    }
}

// y = act(x [m,k] @ w^T + bias + residual), w = nn.Linear weight [n,k] with leading dimension ldw, read in place as
// its transpose when the strided MFMA path takes the shape, through an explicit transpose in `tr` otherwise
struct Lin {
    const float* w; int n, k; int64_t ldw;
    bool in_place() const { return k % 32 == 0 && n % 4 == 0 && ldw % 4 == 0 && ((uintptr_t)w & 15u) == 0; }
    int64_t tr_floats() const { return in_place() ? 0 : (int64_t)k * n; }
};

int linear_fwd(const Lin& l, const float* x, int64_t m, int64_t ldx, const float* bias, const float* residual, int64_t ldr,
               int act, float slope, float* y, float* tr, void* tmp, int64_t tmp_bytes, hipStream_t st)
{
    if (l.in_place())
        return ws_gemm_xb_epilogue_strided(x, m, l.k, ldx, l.w, 1, l.ldw, l.n, bias, residual, ldr, act, slope, y, l.n, tmp, tmp_bytes, st);
    transpose_small_kernel<<<(unsigned)ws_ceil_div((int64_t)l.k * l.n, 256), 256, 0, st>>>(l.w, l.n, l.k, l.ldw, tr);
    return ws_gemm_xb_epilogue_strided(x, m, l.k, ldx, tr, l.n, 1, l.n, bias, residual, ldr, act, slope, y, l.n, tmp, tmp_bytes, st);
}

#define WS_TRY(call)            \
    do {                        \
        int rc__ = (call);      \
        if (rc__) return rc__;  \
    } while (0)

inline bool grouped_rows(int64_t rows) { return ws_block_group_rows > 0 && rows > 0 && rows < ws_block_group_rows; }

inline ws_xb_problem xb_problem(const float* x, int64_t m, int k, int64_t ldx, const float* b, int64_t brs, int64_t bcs, int n,
                                const float* bias, const float* residual, int64_t ldr, int act, float slope, const float* gate_y,
                                int64_t ldg, float gate_slope, float* y, int64_t ldy, void* scratch, int64_t scratch_bytes)
{
    ws_xb_problem q{};
    q.x = x; q.m = m; q.k = k; q.ldx = ldx; q.b = b; q.b_row_stride = brs; q.b_col_stride = bcs; q.n = n;
    q.bias = bias; q.residual = residual; q.ldr = ldr; q.act = act; q.slope = slope;
    q.gate_y = gate_y; q.ldg = ldg; q.gate_slope = gate_slope;
    q.y = y; q.ldy = ldy; q.scratch = scratch; q.scratch_bytes = scratch_bytes;
    return q;
}

// the weight-gradient products of one call: launched one by one where they stand (grouping off), or collected and launched
// together by flush().  Collected members need their operands untouched until flush() and a scratch each.
struct Leaves {
    bool on;
    hipStream_t st;
    ws_xty_problem q[4];
    int n = 0;
    Leaves(bool on_, hipStream_t st_) : on(on_), st(st_) {}
    int add(const float* x, int64_t m, int k, int64_t ldx, const float* y, int nn, int64_t ldy, float* out, int64_t ldo, void* scratch,
            int64_t scratch_bytes)
    {
        if (!on) return ws_priv_gemm_xty_pitched(x, m, k, ldx, y, nn, ldy, out, ldo > nn ? ldo : nn, scratch, st);
        WS_REQUIRE(n < 4, "more than 4 collected weight-gradient products");
        q[n++] = ws_xty_problem{x, m, k, ldx, y, nn, ldy, out, ldo, scratch, scratch_bytes};
        return WS_OK;
    }
    int flush()
    {
        const int c = n;
        n = 0;
        return c ? ws_priv_gemm_xty_group(q, c, st) : WS_OK;
    }
};

// ---- launch timer (bench.py: HIP events around the K3 launch, on the launch stream) --------------------------
struct TimerRec { hipEvent_t a, b, c; int64_t nq; int32_t h, ci; };      // a .. b: the K3 launch, a .. c: K3 + the contraction
std::vector<TimerRec>& timer_recs() { static std::vector<TimerRec> v; return v; }

// the strided block's arg-max record lives in the block's own arena slot (only ws_kpblock_bwd reads it): bytes when the
// neighbour columns fit one (4x fewer bytes for the backward's per-pair reads), the forward and the backward decide alike
bool arg_bytes(const ws_kpblock* d)
{
    return d->h <= 255 && d->in_dim % 4 == 0 && ((uintptr_t)d->feat & 15u) == 0 && ((uintptr_t)d->pooled & 15u) == 0 &&
           ((uintptr_t)d->arg & 3u) == 0;
}

int check_kpblock(const ws_kpblock* d)
{
    WS_REQUIRE(d, "NULL descriptor");
    WS_REQUIRE(d->nq >= 0 && d->ns >= 0 && d->h >= 1, "bad sizes nq=%lld ns=%lld h=%d", (long long)d->nq, (long long)d->ns, d->h);
    if (!ws_kpconv_supported_k(d->k, 0, 0))
        return ws_fail(WS_ERR_UNSUPPORTED, "num_kernel_points=%d: this build instantiates K=9, K=13 and K=15", d->k);
    WS_REQUIRE(d->k == 15 || d->wf, "wf buffer missing (the one-launch forward layer is built for K = 15 only)");
    WS_REQUIRE(d->in_dim >= 1 && d->conv_in >= 1 && d->conv_out >= 1 && d->out_dim >= 1, "bad widths");
    WS_REQUIRE(d->q_pts && d->s_pts && d->inds && d->kernel_points && d->feat && d->wk && (d->wf || d->infer) && d->out, "NULL argument");
    WS_REQUIRE(d->w1 ? (d->x1 != nullptr) : (d->conv_in == d->in_dim), "unary1: x1 buffer missing or conv_in != in_dim");
    WS_REQUIRE(d->w2 ? (d->x2 != nullptr) : (d->out_dim == d->conv_out), "unary2: x2 buffer missing or out_dim != conv_out");
    WS_REQUIRE(!d->w2 || d->ws || d->in_dim == d->out_dim, "shortcut needs a projection (ws) when in_dim != out_dim");
    WS_REQUIRE(!d->strided || !d->w2 || (d->pooled && d->arg), "strided block: pooled / arg buffers missing");
    WS_REQUIRE(d->strided || d->nq == d->ns, "non-strided block: nq must equal ns");
    // queries without a single support: the forward would be act(bias) rows whose bias gradients are live -- no caller sends it
    if (d->ns == 0 && d->nq > 0)
        return ws_fail(WS_ERR_UNSUPPORTED, "block with queries but no supports (nq=%lld ns=%lld)", (long long)d->nq, (long long)d->ns);
    if (d->conv_out % 4 || d->out_dim % 4 || (d->w1 && d->conv_in % 4) || (d->w2 && d->in_dim % 4))
        return ws_fail(WS_ERR_UNSUPPORTED, "block widths must be multiples of 4 (in=%d conv=%d->%d out=%d)", d->in_dim, d->conv_in,
                       d->conv_out, d->out_dim);
    return WS_OK;
}

int64_t kpblock_tmp_fwd(const ws_kpblock* d)
{
    int64_t t = ws_gemm_xb_scratch_bytes(d->nq, d->k * d->conv_in, d->conv_out);
    if (d->w1) t = max3(t, ws_gemm_xb_scratch_bytes(d->ns, d->in_dim, d->conv_in), 0);
    if (d->w2) t = max3(t, ws_gemm_xb_scratch_bytes(d->nq, d->conv_out, d->out_dim), d->ws ? ws_gemm_xb_scratch_bytes(d->nq, d->in_dim, d->out_dim) : 0);
    return t;
}

int kpblock_fwd(const ws_kpblock* d, Arena& ar, hipStream_t st, bool run)
{
    const int64_t nq = d->nq, ns = d->ns;
    const Lin l1{d->w1, d->conv_in, d->in_dim, d->in_dim}, l2{d->w2, d->out_dim, d->conv_out, d->conv_out},
        lsc{d->ws, d->out_dim, d->in_dim, d->in_dim};
    float* tr1 = d->w1 ? ar.take<float>(l1.tr_floats()) : nullptr;
    float* tr2 = d->w2 ? ar.take<float>(l2.tr_floats()) : nullptr;
    float* trs = d->ws ? ar.take<float>(lsc.tr_floats()) : nullptr;
    float* sc = (d->w2 && d->ws) ? ar.take<float>(nq * d->out_dim) : nullptr;
    const int64_t tmp_bytes = kpblock_tmp_fwd(d);
    void* tmp = ar.take<char>(tmp_bytes > 16 ? tmp_bytes : 16);
    // unary1 (feat -> x1) and the shortcut projection (feat -> sc) of a non-strided block read the same rows: one grouped
    // launch, the projection with a split-K scratch of its own
    const bool pair_in = grouped_rows(nq) && d->w1 && d->w2 && d->ws && !d->strided && l1.in_place() && lsc.in_place();
    const int64_t sc_bytes = pair_in ? ws_gemm_xb_scratch_bytes(nq, d->in_dim, d->out_dim) : 0;
    void* tmp_sc = pair_in ? (void*)ar.take<char>(sc_bytes > 16 ? sc_bytes : 16) : nullptr;
    if (!run) return WS_OK;
    if (nq == 0) return WS_OK;
    const float* x1 = d->feat;
    if (pair_in) {
        const ws_xb_problem q[2] = {
            xb_problem(d->feat, ns, l1.k, d->in_dim, l1.w, 1, l1.ldw, l1.n, d->b1, nullptr, 0, 1, d->slope, nullptr, 0, 0.0f, d->x1, l1.n,
                       tmp, tmp_bytes),
            xb_problem(d->feat, nq, lsc.k, d->in_dim, lsc.w, 1, lsc.ldw, lsc.n, d->bs, nullptr, 0, 0, 0.0f, nullptr, 0, 0.0f, sc, lsc.n,
                       tmp_sc, sc_bytes)};
        WS_TRY(ws_priv_gemm_xb_group(q, 2, st));
        x1 = d->x1;
    } else if (d->w1) {
        WS_TRY(linear_fwd(l1, d->feat, ns, d->in_dim, d->b1, nullptr, 0, 1, d->slope, d->x1, tr1, tmp, tmp_bytes, st));
        x1 = d->x1;
    }
    TimerRec rec{};
    if (d->timed) {
        WS_HIP(hipEventCreate(&rec.a));
        WS_HIP(hipEventCreate(&rec.b));
        rec.nq = nq; rec.h = d->h; rec.ci = d->conv_in;
        WS_HIP(hipEventRecord(rec.a, st));
    }
    float* x2 = d->w2 ? d->x2 : d->out;
    // forward only and a layer the one-launch kernel covers: the contraction runs inside the gather, no `wf`
    const bool one_launch = d->infer && d->k == 15 && d->conv_in == 32 && d->conv_out == 32 && !d->rows_sorted && ((uintptr_t)x1 & 15u) == 0 &&
                            ((uintptr_t)d->wk & 15u) == 0 && ((uintptr_t)x2 & 15u) == 0 && ws_block_fused_infer;
    if (one_launch) {
        WS_TRY(ws_kpconv_layer_fwd_fused(d->q_pts, nq, d->s_pts, ns, d->inds, d->h, x1, d->conv_in, d->kernel_points, d->k, d->extent,
                                         d->order_q, d->wk, d->conv_out, d->bk, 1, d->slope, x2, st));
        if (d->timed) WS_HIP(hipEventRecord(rec.b, st));
    } else {
        WS_REQUIRE(d->wf, "wf buffer missing");
        WS_TRY(ws_kpconv_gather_fwd_ex(d->q_pts, nq, d->s_pts, ns, d->inds, d->h, x1, d->conv_in, d->kernel_points, d->k, nullptr,
                                       nullptr, d->extent, WS_INFLUENCE_LINEAR, WS_AGGREGATION_SUM, d->order_q, d->wf, nullptr, 0,
                                       d->rows_sorted, st));
        if (d->timed) WS_HIP(hipEventRecord(rec.b, st));
        WS_TRY(ws_gemm_xb_epilogue_strided(d->wf, nq, d->k * d->conv_in, (int64_t)d->k * d->conv_in, d->wk, d->conv_out, 1, d->conv_out,
                                           d->bk, nullptr, 0, 1, d->slope, x2, d->conv_out, tmp, tmp_bytes, st));
    }
    if (d->timed) {
        WS_HIP(hipEventCreate(&rec.c));
        WS_HIP(hipEventRecord(rec.c, st));
        timer_recs().push_back(rec);
    }
    if (!d->w2) return WS_OK;
    const float* sc_in = d->feat;
    if (d->strided) {
        if (arg_bytes(d))
            WS_TRY(ws_priv_max_pool_fwd_u8(d->feat, ns, d->in_dim, d->inds, nq, d->h, d->pooled, reinterpret_cast<uint8_t*>(d->arg),
                                           ws_block_pool_order ? d->order_q : nullptr, st));
        else
            WS_TRY(ws_max_pool_fwd(d->feat, ns, d->in_dim, d->inds, nq, d->h, d->pooled, d->arg, st));
        sc_in = d->pooled;
    }
    const float* res = sc_in;
    int64_t ldr = d->in_dim;
    if (d->ws) {
        if (!pair_in) WS_TRY(linear_fwd(lsc, sc_in, nq, d->in_dim, d->bs, nullptr, 0, 0, 0.0f, sc, trs, tmp, tmp_bytes, st));
        res = sc;
        ldr = d->out_dim;
    }
    return linear_fwd(l2, x2, nq, d->conv_out, d->b2, res, ldr, 1, d->slope, d->out, tr2, tmp, tmp_bytes, st);
}

int kpblock_bwd(const ws_kpblock* d, Arena& ar, hipStream_t st, bool run)
{
    const int64_t nq = d->nq, ns = d->ns;
    const int kc = d->k * d->conv_in;
    const bool need_dx1 = d->dfeat != nullptr || d->w1 != nullptr;
    const bool want_sc = d->w2 && d->dfeat;                       // the shortcut's share of dfeat
    // ---- arena plan (identical in the size query and in the run)
    float* dz = d->w2 ? ar.take<float>(nq * d->out_dim) : nullptr;
    float* g2 = ar.take<float>(nq * d->conv_out);                  // dx2 -> dz2 (simple block: dz2 of dout)
    float* dwf = need_dx1 ? ar.take<float>(nq * (int64_t)kc) : nullptr;
    float* dx1 = (need_dx1 && d->w1) ? ar.take<float>(ns * d->conv_in) : nullptr;
    float* dscin = (want_sc && d->ws) ? ar.take<float>(nq * d->in_dim) : nullptr;
    float* dfsc = (want_sc && d->strided) ? ar.take<float>(ns * d->in_dim) : nullptr;
    const Lin lk{d->wk, kc, d->conv_out, d->conv_out};           // dwf = dz2 @ wk^T: wk [kc, conv_out] read as a "Linear" weight
    float* trk = need_dx1 ? ar.take<float>(lk.tr_floats()) : nullptr;
    int64_t tmp_bytes = max3(ws_act_bwd_colsum_scratch_bytes(nq, d->out_dim > d->conv_out ? d->out_dim : d->conv_out),
                             ws_act_bwd_colsum_scratch_bytes(ns, d->conv_in), ws_gemm_xty_scratch_bytes(nq, kc, d->conv_out));
    if (d->w2) tmp_bytes = max3(tmp_bytes, ws_gemm_xty_scratch_bytes(nq, d->out_dim, d->conv_out),
                                d->ws ? ws_gemm_xty_scratch_bytes(nq, d->out_dim, d->in_dim) : 0);
    if (d->w1) tmp_bytes = max3(tmp_bytes, ws_gemm_xty_scratch_bytes(ns, d->conv_in, d->in_dim), 0);
    tmp_bytes = max3(tmp_bytes, ws_gemm_xb_scratch_bytes(nq, d->conv_out, kc), ws_gemm_xb_scratch_bytes(nq, d->out_dim, d->conv_out));
    tmp_bytes = max3(tmp_bytes, ws_gemm_xb_scratch_bytes(nq, d->out_dim, d->in_dim), ws_gemm_xb_scratch_bytes(ns, d->conv_in, d->in_dim));
    void* tmp = ar.take<char>(tmp_bytes > 16 ? tmp_bytes : 16);
    // grouped: the collected weight-gradient products and the second member of the dz pair take a scratch each (a sum
    // where the single launches share the maximum); the operands the collected products read -- dz (or dout when
    // pregated), g2, dx1, wf, x2, feat, pooled -- stay untouched until the end of the call
    const bool grp = grouped_rows(nq > ns ? nq : ns) && nq > 0 && ns > 0;
    const int64_t b_dwk = ws_gemm_xty_scratch_bytes(nq, kc, d->conv_out);
    const int64_t b_dw2 = d->w2 ? ws_gemm_xty_scratch_bytes(nq, d->out_dim, d->conv_out) : 0;
    const int64_t b_dws = (d->w2 && d->ws) ? ws_gemm_xty_scratch_bytes(nq, d->out_dim, d->in_dim) : 0;
    const int64_t b_dw1 = d->w1 ? ws_gemm_xty_scratch_bytes(ns, d->conv_in, d->in_dim) : 0;
    const int64_t b_g2 = d->w2 ? ws_gemm_xb_scratch_bytes(nq, d->out_dim, d->conv_out) : 0;
    auto own = [&](int64_t bytes) -> void* { return grp ? (void*)ar.take<char>(bytes > 16 ? bytes : 16) : tmp; };
    void* t_dwk = own(b_dwk);
    void* t_dw2 = d->w2 ? own(b_dw2) : tmp;
    void* t_dws = (d->w2 && d->ws) ? own(b_dws) : tmp;
    void* t_dw1 = d->w1 ? own(b_dw1) : tmp;
    void* t_g2 = d->w2 ? own(b_g2) : tmp;
    if (!run) return WS_OK;
    WS_REQUIRE(d->dout && d->dwk, "NULL gradient buffer");
    WS_REQUIRE(!d->w1 || d->dw1, "dw1 missing");
    WS_REQUIRE(!d->w2 || d->dw2, "dw2 missing");
    WS_REQUIRE(!d->ws || !d->w2 || d->dws, "dws missing");
    if (nq == 0) {
        // no output rows (ns == 0 with nq > 0 is refused by check_kpblock): every gradient is zero
        WS_HIP(hipMemsetAsync(d->dwk, 0, sizeof(float) * (size_t)kc * d->conv_out, st));
        if (d->dbk) WS_HIP(hipMemsetAsync(d->dbk, 0, sizeof(float) * d->conv_out, st));
        if (d->w1) { WS_HIP(hipMemsetAsync(d->dw1, 0, sizeof(float) * (size_t)d->conv_in * d->in_dim, st)); if (d->db1) WS_HIP(hipMemsetAsync(d->db1, 0, sizeof(float) * d->conv_in, st)); }
        if (d->w2) { WS_HIP(hipMemsetAsync(d->dw2, 0, sizeof(float) * (size_t)d->out_dim * d->conv_out, st)); if (d->db2) WS_HIP(hipMemsetAsync(d->db2, 0, sizeof(float) * d->out_dim, st)); }
        if (d->w2 && d->ws) WS_HIP(hipMemsetAsync(d->dws, 0, sizeof(float) * (size_t)d->out_dim * d->in_dim, st));
        if (d->dfeat && ns > 0) {
            if (d->dfeat_add) WS_HIP(hipMemcpyAsync(d->dfeat, d->dfeat_add, sizeof(float) * (size_t)ns * d->in_dim, hipMemcpyDeviceToDevice, st));
            else WS_HIP(hipMemsetAsync(d->dfeat, 0, sizeof(float) * (size_t)ns * d->in_dim, st));
        }
        return WS_OK;
    }
    bool gated2 = false;
    Leaves leaves(grp, st);
    const float* sc_res = nullptr;          // the shortcut's gradient w.r.t. feat rows [ns,in_dim]
    bool added = false;                     // dfeat_add already summed in (by the pool backward's store)
    const float* gin = d->dout;             // gradient entering the convolution's activation
    const float* yconv = d->out;
    WS_REQUIRE(!(d->gate_dfeat && d->dfeat_add && !(d->strided && want_sc)),
               "gate_dfeat with dfeat_add needs the strided shortcut (the sum has to be complete before the gate)");
    if (d->w2) {
        // dz = dout * lrelu'(out), db2 = column sums (dout_pregated: the consumer has done the multiplication)
        if (d->dout_pregated) {
            if (d->db2) WS_TRY(ws_act_bwd_colsum(d->dout, nq, d->out_dim, d->out_dim, nullptr, 0, 0.0f, nullptr, 0, d->db2, tmp, st));
            dz = const_cast<float*>(d->dout);          // (read only from here on)
        } else
        WS_TRY(ws_act_bwd_colsum(d->dout, nq, d->out_dim, d->out_dim, d->out, d->out_dim, d->slope, dz, d->out_dim, d->db2, tmp, st));
        WS_TRY(leaves.add(dz, nq, d->out_dim, d->out_dim, d->x2, d->conv_out, d->conv_out, d->dw2, 0, t_dw2, b_dw2));
        if (d->ws) {
            const float* sc_in = d->strided ? d->pooled : d->feat;
            WS_TRY(leaves.add(dz, nq, d->out_dim, d->out_dim, sc_in, d->in_dim, d->in_dim, d->dws, 0, t_dws, b_dws));
        }
        // dx2 = dz @ w2; without a bias gradient to sum (use_bn: BatchNormBlock is an identity, blocks.py:453-463) the
        // activation backward of the convolution's LeakyReLU rides on the epilogue: dz2 = dx2 * lrelu'(x2)
        gated2 = !d->dbk && ws_block_gates;
        // grouped: dscin = dz @ ws and g2 = dz @ w2 both wait for dz only -- one launch, one split epilogue
        const bool pair_dz = grp && want_sc && d->ws;
        if (pair_dz) {
            const ws_xb_problem q[2] = {
                xb_problem(dz, nq, d->out_dim, d->out_dim, d->ws, d->in_dim, 1, d->in_dim, nullptr, nullptr, 0, 0, 0.0f, nullptr, 0, 0.0f,
                           dscin, d->in_dim, tmp, tmp_bytes),
                xb_problem(dz, nq, d->out_dim, d->out_dim, d->w2, d->conv_out, 1, d->conv_out, nullptr, nullptr, 0, 0, 0.0f,
                           gated2 ? d->x2 : nullptr, d->conv_out, d->slope, g2, d->conv_out, t_g2, b_g2)};
            WS_TRY(ws_priv_gemm_xb_group(q, 2, st));
        }
        if (want_sc) {
            const float* dsc = dz;          // [nq, in_dim] when there is no projection (in_dim == out_dim)
            if (d->ws) {
                if (!pair_dz)
                    WS_TRY(ws_gemm_xb_epilogue_strided(dz, nq, d->out_dim, d->out_dim, d->ws, d->in_dim, 1, d->in_dim, nullptr, nullptr, 0,
                                                       0, 0.0f, dscin, d->in_dim, tmp, tmp_bytes, st));
                dsc = dscin;
            }
            if (d->strided) {
                WS_REQUIRE(d->t_offsets && d->t_pairs, "strided block backward needs the transposed table");
                if (arg_bytes(d))
                {
                    WS_TRY(ws_priv_max_pool_bwd_u8(dsc, reinterpret_cast<const uint8_t*>(d->arg), nq, d->h, d->in_dim, d->t_offsets,
                                                   d->t_pairs, ns, dfsc, ws_block_pool_order ? d->order_s : nullptr, d->dfeat_add, st));
                    added = d->dfeat_add != nullptr;
                }
                else {
                    WS_TRY(ws_max_pool_bwd(dsc, d->arg, nq, d->h, d->in_dim, d->t_offsets, d->t_pairs, ns, dfsc, st));
                    if (d->dfeat_add) {
                        WS_REQUIRE(d->in_dim % 4 == 0, "dfeat_add needs in_dim %% 4 == 0");
                        const int64_t n4 = ns * d->in_dim / 4;
                        add_rows_kernel<<<ws_grid(n4, 256), 256, 0, st>>>(dfsc, d->dfeat_add, n4);
                        WS_LAUNCH_CHECK();
                        added = true;
                    }
                }
                sc_res = dfsc;
            } else {
                sc_res = dsc;
            }
        }
        if (!pair_dz)
            WS_TRY(ws_gemm_xb_gated_strided(dz, nq, d->out_dim, d->out_dim, d->w2, d->conv_out, 1, d->conv_out, nullptr, nullptr, 0, 0, 0.0f,
                                            gated2 ? d->x2 : nullptr, d->conv_out, d->slope, nullptr, 0, 0.0f, g2, d->conv_out, tmp,
                                            tmp_bytes, st));
        gin = g2;
        yconv = d->x2;
    }
    // dz2 = g * lrelu'(x2), dbk
    if (!d->w2 && d->dout_pregated) {          // simple block whose consumer has applied the LeakyReLU' already
        if (d->dbk) WS_TRY(ws_act_bwd_colsum(gin, nq, d->conv_out, d->conv_out, nullptr, 0, 0.0f, nullptr, 0, d->dbk, tmp, st));
        g2 = const_cast<float*>(gin);              // (read only from here on)
    } else if (!gated2)
        WS_TRY(ws_act_bwd_colsum(gin, nq, d->conv_out, d->conv_out, yconv, d->conv_out, d->slope, g2, d->conv_out, d->dbk, tmp, st));
    WS_TRY(leaves.add(d->wf, nq, kc, kc, g2, d->conv_out, d->conv_out, d->dwk, 0, t_dwk, b_dwk));
    if (!need_dx1) return leaves.flush();
    // dwf = dz2 @ wk^T
    WS_TRY(linear_fwd(lk, g2, nq, d->conv_out, nullptr, nullptr, 0, 0, 0.0f, dwf, trk, tmp, tmp_bytes, st));
    float* dx1_out = d->w1 ? dx1 : d->dfeat;
    // unary1's LeakyReLU backward rides on the store of K4 / K4G when no bias gradient has to be summed from dz1
    const float* gate1 = (d->w1 && !d->db1 && ws_block_gates) ? d->x1 : nullptr;
    if (!d->w1 && d->gate_dfeat && d->dfeat) gate1 = d->feat;   // no unary1: K4 / K4G writes dfeat itself -- times LeakyReLU'(feat)
    if (d->grid_blob) {
        WS_REQUIRE(d->key_last && d->grid_overflow && nq == ns, "grid backward needs key_last / overflow and a self-query layer");
        WS_TRY(ws_kpconv_gather_bwd_x_grid_gated(d->s_pts, ns, d->grid_blob, d->grid_nb, d->grid_cells, d->key_last, d->grid_radius, dwf,
                                                 d->conv_in, d->kernel_points, d->k, nullptr, nullptr, d->extent, WS_INFLUENCE_LINEAR,
                                                 WS_AGGREGATION_SUM, d->order_s, gate1, d->slope, d->inds, d->h, dx1_out,
                                                 d->grid_overflow, st));
    } else {
        WS_REQUIRE(d->t_offsets && d->t_pairs, "KPConv backward needs the search grid or the transposed table");
        // (the strided blocks: four supports per wave where the packed form applies, the same dx bit for bit)
        WS_TRY((ws_block_packed_k4 ? ws_kpconv_gather_bwd_x_packed : ws_kpconv_gather_bwd_x_gated)(
            d->q_pts, nq, d->s_pts, ns, d->inds, d->h, d->t_offsets, d->t_pairs, dwf, d->conv_in, d->kernel_points, d->k, nullptr, nullptr,
            d->extent, WS_INFLUENCE_LINEAR, WS_AGGREGATION_SUM, d->order_s, gate1, d->slope, dx1_out, st));
    }
    if (d->w1) {
        if (!gate1)
            WS_TRY(ws_act_bwd_colsum(dx1, ns, d->conv_in, d->conv_in, d->x1, d->conv_in, d->slope, dx1, d->conv_in, d->db1, tmp, st));
        WS_TRY(leaves.add(dx1, ns, d->conv_in, d->conv_in, d->feat, d->in_dim, d->in_dim, d->dw1, 0, t_dw1, b_dw1));
        if (d->dfeat)
            WS_TRY(ws_gemm_xb_gated_strided(dx1, ns, d->conv_in, d->conv_in, d->w1, d->in_dim, 1, d->in_dim, nullptr, sc_res, d->in_dim,
                                            0, 0.0f, d->gate_dfeat ? d->feat : nullptr, d->in_dim, d->slope, nullptr, 0, 0.0f, d->dfeat,
                                            d->in_dim, tmp, tmp_bytes, st));
    } else if (d->dfeat && sc_res) {
        WS_REQUIRE(!d->gate_dfeat, "gate_dfeat: a block without unary1 has no shortcut to add after the gate");
        const int64_t n4 = ns * d->in_dim / 4;
        add_rows_kernel<<<ws_grid(n4, 256), 256, 0, st>>>(d->dfeat, sc_res, n4);
        WS_LAUNCH_CHECK();
    }
    if (d->dfeat && d->dfeat_add && !added) {       // (block shapes without a strided shortcut: a pass of its own)
        WS_REQUIRE(d->in_dim % 4 == 0, "dfeat_add needs in_dim %% 4 == 0");
        const int64_t n4 = ns * d->in_dim / 4;
        add_rows_kernel<<<ws_grid(n4, 256), 256, 0, st>>>(d->dfeat, d->dfeat_add, n4);
        WS_LAUNCH_CHECK();
    }
    return leaves.flush();
}

// ---- decoder step ------------------------------------------------------------------------------------------------
int check_upunary(const ws_upunary* d)
{
    WS_REQUIRE(d, "NULL descriptor");
    WS_REQUIRE(d->nc >= 0 && d->nf >= 0 && d->c_up >= 1 && d->c_skip >= 1 && d->out_dim >= 1 && d->h_up >= 1, "bad sizes");
    WS_REQUIRE(d->xc && d->skip && d->ups && d->w && d->out && d->ldw >= d->c_up + d->c_skip, "NULL argument / bad ldw");
    if (d->c_up % 32 || d->c_skip % 32 || d->out_dim % 32 || d->ldw % 4 || ((uintptr_t)d->w & 15u))
        return ws_fail(WS_ERR_UNSUPPORTED, "decoder step: widths must be multiples of 32 (c_up=%d c_skip=%d out=%d)", d->c_up, d->c_skip,
                       d->out_dim);
    WS_REQUIRE(d->drop_p >= 0.0f && d->drop_p < 1.0f, "bad drop probability %g", (double)d->drop_p);
    if (d->drop_p > 0.0f && !d->relu) return ws_fail(WS_ERR_UNSUPPORTED, "decoder step: the fused dropout follows a LeakyReLU (relu = 0)");
    WS_REQUIRE(!(d->dout_pregated && !d->relu), "dout_pregated needs this step's LeakyReLU");
    // fine rows without a single coarse row: out = act(skip @ Ws^T + b), whose gradients are live -- no caller sends it
    if (d->nc == 0 && d->nf > 0)
        return ws_fail(WS_ERR_UNSUPPORTED, "decoder step with fine rows but no coarse rows (nc=%lld nf=%lld)", (long long)d->nc, (long long)d->nf);
    return WS_OK;
}

int upunary_fwd(const ws_upunary* d, Arena& ar, hipStream_t st, bool run)
{
    float* up = ar.take<float>(d->nf * d->out_dim);
    const int64_t tmp_bytes = max3(ws_gemm_xb_scratch_bytes(d->nc, d->c_up, d->out_dim), ws_gemm_xb_scratch_bytes(d->nf, d->c_skip, d->out_dim), 16);
    void* tmp = ar.take<char>(tmp_bytes);
    if (!run || d->nf == 0) return WS_OK;
    WS_REQUIRE(d->yc, "yc buffer missing");
    // (nf > 0 here, so nc > 0: check_upunary refuses fine rows without coarse rows)
    WS_TRY(ws_gemm_xb_epilogue_strided(d->xc, d->nc, d->c_up, d->c_up, d->w, 1, d->ldw, d->out_dim, nullptr, nullptr, 0, 0, 0.0f, d->yc,
                                       d->out_dim, tmp, tmp_bytes, st));
    if (ws_block_gather_residual)
        // nearest upsampling (closest_pool) read by the epilogue: out row r adds yc[ups[r, 0]] (nothing for the shadow index);
        // the droplayer in front of the head (drop_p > 0) rides on the same epilogue
        return ws_priv_gemm_xb_ex(d->skip, d->nf, d->c_skip, d->c_skip, d->w + d->c_up, 1, d->ldw, d->out_dim, d->b, d->yc, d->out_dim,
                                  d->ups, d->h_up, d->nc, d->relu ? 1 : 0, d->slope, d->drop_p, d->drop_seed, d->out, d->out_dim, tmp,
                                  tmp_bytes, st);
    WS_TRY(ws_closest_pool_fwd(d->yc, d->nc, d->out_dim, d->ups, d->nf, d->h_up, up, st));
    if (d->drop_p > 0.0f)
        return ws_gemm_xb_dropout_strided(d->skip, d->nf, d->c_skip, d->c_skip, d->w + d->c_up, 1, d->ldw, d->out_dim, d->b, up, d->out_dim,
                                          1, d->slope, d->drop_p, d->drop_seed, d->out, d->out_dim, tmp, tmp_bytes, st);
    return ws_gemm_xb_epilogue_strided(d->skip, d->nf, d->c_skip, d->c_skip, d->w + d->c_up, 1, d->ldw, d->out_dim, d->b, up, d->out_dim,
                                       d->relu ? 1 : 0, d->slope, d->out, d->out_dim, tmp, tmp_bytes, st);
}

int upunary_bwd(const ws_upunary* d, Arena& ar, hipStream_t st, bool run)
{
    float* dz = ar.take<float>(d->nf * d->out_dim);
    float* dyc = ar.take<float>(d->nc * d->out_dim);
    int64_t tmp_bytes = max3(ws_act_bwd_colsum_scratch_bytes(d->nf, d->out_dim), ws_gemm_xty_scratch_bytes(d->nf, d->out_dim, d->c_skip),
                             ws_gemm_xty_scratch_bytes(d->nc, d->out_dim, d->c_up));
    tmp_bytes = max3(tmp_bytes, ws_gemm_xb_scratch_bytes(d->nf, d->out_dim, d->c_skip), ws_gemm_xb_scratch_bytes(d->nc, d->out_dim, d->c_up));
    void* tmp = ar.take<char>(tmp_bytes > 16 ? tmp_bytes : 16);
    // grouped: the two pitched halves of dw are leaves -- collected, launched together at the end, a scratch each
    const bool grp = grouped_rows(d->nf > d->nc ? d->nf : d->nc) && d->nf > 0 && d->nc > 0;
    const int64_t b_skip = ws_gemm_xty_scratch_bytes(d->nf, d->out_dim, d->c_skip), b_up = ws_gemm_xty_scratch_bytes(d->nc, d->out_dim, d->c_up);
    void* t_skip = grp ? (void*)ar.take<char>(b_skip > 16 ? b_skip : 16) : tmp;
    void* t_up = grp ? (void*)ar.take<char>(b_up > 16 ? b_up : 16) : tmp;
    if (!run) return WS_OK;
    WS_REQUIRE(d->dout && d->dw && d->dxc && d->dskip && d->t_offsets && d->t_pairs, "NULL gradient buffer / table");
    const int64_t cw = d->c_up + d->c_skip;
    if (d->nf == 0) {
        // no output rows (nc == 0 with nf > 0 is refused by check_upunary): every gradient is zero
        WS_HIP(hipMemsetAsync(d->dw, 0, sizeof(float) * (size_t)d->out_dim * cw, st));
        if (d->db) WS_HIP(hipMemsetAsync(d->db, 0, sizeof(float) * d->out_dim, st));
        if (d->nc > 0) WS_HIP(hipMemsetAsync(d->dxc, 0, sizeof(float) * (size_t)d->nc * d->c_up, st));
        return WS_OK;
    }
    // dz = dout * lrelu'(out) (identity when !relu), db
    const float* g = d->dout;
    if (d->relu && d->dout_pregated) {             // the consumer has applied this step's LeakyReLU' (and dropout backward) already
        if (d->db) WS_TRY(ws_act_bwd_colsum(d->dout, d->nf, d->out_dim, d->out_dim, nullptr, 0, 0.0f, nullptr, 0, d->db, tmp, st));
    } else if (d->drop_p > 0.0f) {
        WS_TRY(ws_act_bwd_colsum_dropout(d->dout, d->nf, d->out_dim, d->out_dim, d->out, d->out_dim, d->slope, d->drop_p, d->drop_seed, dz,
                                         d->out_dim, d->db, tmp, st));
        g = dz;
    } else if (d->relu) {
        WS_TRY(ws_act_bwd_colsum(d->dout, d->nf, d->out_dim, d->out_dim, d->out, d->out_dim, d->slope, dz, d->out_dim, d->db, tmp, st));
        g = dz;
    } else if (d->db) {
        WS_TRY(ws_act_bwd_colsum(d->dout, d->nf, d->out_dim, d->out_dim, nullptr, 0, 0.0f, nullptr, 0, d->db, tmp, st));
    }
    // skip side
    // (the two halves of dw [out, c_up + c_skip] are written in place: column blocks of pitch cw)
    Leaves leaves(grp, (hipStream_t)st);
    WS_TRY(leaves.add(g, d->nf, d->out_dim, d->out_dim, d->skip, d->c_skip, d->c_skip, d->dw + d->c_up, cw, t_skip, b_skip));
    WS_TRY(ws_gemm_xb_epilogue_strided(g, d->nf, d->out_dim, d->out_dim, d->w + d->c_up, d->ldw, 1, d->c_skip, nullptr, nullptr, 0, 0, 0.0f,
                                       d->dskip, d->c_skip, tmp, tmp_bytes, st));
    // coarse side: nearest upsampling backward, then the x-part of the unary
    WS_TRY(ws_closest_pool_bwd(g, d->nf, 1, d->out_dim, d->t_offsets, d->t_pairs, d->nc, dyc, st));
    WS_TRY(leaves.add(dyc, d->nc, d->out_dim, d->out_dim, d->xc, d->c_up, d->c_up, d->dw, cw, t_up, b_up));
    WS_TRY(ws_gemm_xb_gated_strided(dyc, d->nc, d->out_dim, d->out_dim, d->w, d->ldw, 1, d->c_up, nullptr, nullptr, 0, 0, 0.0f,
                                    d->gate_dxc ? d->xc : nullptr, d->c_up, d->slope, nullptr, 0, 0.0f, d->dxc, d->c_up, tmp, tmp_bytes, st));
    return leaves.flush();
}

}  // namespace

extern "C" {

int64_t ws_kpblock_bytes(void) { return (int64_t)sizeof(ws_kpblock); }
int64_t ws_upunary_bytes(void) { return (int64_t)sizeof(ws_upunary); }

int64_t ws_kpblock_fwd_scratch_bytes(const ws_kpblock* d)
{
    if (check_kpblock(d)) return -1;
    Arena ar(nullptr, 0);
    kpblock_fwd(d, ar, nullptr, false);
    return arena_bytes(ar);
}

int64_t ws_kpblock_bwd_scratch_bytes(const ws_kpblock* d)
{
    if (check_kpblock(d)) return -1;
    Arena ar(nullptr, 0);
    kpblock_bwd(d, ar, nullptr, false);
    return arena_bytes(ar);
}

int ws_kpblock_fwd(const ws_kpblock* d, void* scratch, int64_t scratch_bytes, void* stream)
{
    WS_TRY(check_kpblock(d));
    WS_REQUIRE(scratch && ((uintptr_t)scratch & 15u) == 0, "scratch must be a 16-byte aligned device buffer");
    Arena plan(nullptr, 0);
    kpblock_fwd(d, plan, nullptr, false);
    if (arena_bytes(plan) > scratch_bytes) return ws_fail(WS_ERR_CAPACITY, "scratch too small: %lld < %lld bytes", (long long)scratch_bytes, (long long)arena_bytes(plan));
    Arena ar(scratch, scratch_bytes);
    return kpblock_fwd(d, ar, (hipStream_t)stream, true);
}

int ws_kpblock_bwd(const ws_kpblock* d, void* scratch, int64_t scratch_bytes, void* stream)
{
    WS_TRY(check_kpblock(d));
    WS_REQUIRE(scratch && ((uintptr_t)scratch & 15u) == 0, "scratch must be a 16-byte aligned device buffer");
    Arena plan(nullptr, 0);
    kpblock_bwd(d, plan, nullptr, false);
    if (arena_bytes(plan) > scratch_bytes) return ws_fail(WS_ERR_CAPACITY, "scratch too small: %lld < %lld bytes", (long long)scratch_bytes, (long long)arena_bytes(plan));
    Arena ar(scratch, scratch_bytes);
    return kpblock_bwd(d, ar, (hipStream_t)stream, true);
}

int64_t ws_upunary_fwd_scratch_bytes(const ws_upunary* d)
{
    if (check_upunary(d)) return -1;
    Arena ar(nullptr, 0);
    upunary_fwd(d, ar, nullptr, false);
    return arena_bytes(ar);
}

int64_t ws_upunary_bwd_scratch_bytes(const ws_upunary* d)
{
    if (check_upunary(d)) return -1;
    Arena ar(nullptr, 0);
    upunary_bwd(d, ar, nullptr, false);
    return arena_bytes(ar);
}

int ws_upunary_fwd(const ws_upunary* d, void* scratch, int64_t scratch_bytes, void* stream)
{
    WS_TRY(check_upunary(d));
    WS_REQUIRE(scratch && ((uintptr_t)scratch & 15u) == 0, "scratch must be a 16-byte aligned device buffer");
    Arena plan(nullptr, 0);
    upunary_fwd(d, plan, nullptr, false);
    if (arena_bytes(plan) > scratch_bytes) return ws_fail(WS_ERR_CAPACITY, "scratch too small: %lld < %lld bytes", (long long)scratch_bytes, (long long)arena_bytes(plan));
    Arena ar(scratch, scratch_bytes);
    return upunary_fwd(d, ar, (hipStream_t)stream, true);
}

int ws_upunary_bwd(const ws_upunary* d, void* scratch, int64_t scratch_bytes, void* stream)
{
    WS_TRY(check_upunary(d));
    WS_REQUIRE(scratch && ((uintptr_t)scratch & 15u) == 0, "scratch must be a 16-byte aligned device buffer");
    Arena plan(nullptr, 0);
    upunary_bwd(d, plan, nullptr, false);
    if (arena_bytes(plan) > scratch_bytes) return ws_fail(WS_ERR_CAPACITY, "scratch too small: %lld < %lld bytes", (long long)scratch_bytes, (long long)arena_bytes(plan));
    Arena ar(scratch, scratch_bytes);
    return upunary_bwd(d, ar, (hipStream_t)stream, true);
}

int ws_timer_reset(void)
{
    for (auto& r : timer_recs()) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
        (void)hipEventDestroy(r.c);
    }
    timer_recs().clear();
    return WS_OK;
}

int ws_timer_count(void) { return (int)timer_recs().size(); }

int ws_timer_read(int32_t i, int64_t* nq, int32_t* h, int32_t* ci, float* ms)
{
    WS_REQUIRE(i >= 0 && i < (int)timer_recs().size() && nq && h && ci && ms, "bad timer record index %d", i);
    const TimerRec& r = timer_recs()[i];
    WS_HIP(hipEventSynchronize(r.b));
    WS_HIP(hipEventElapsedTime(ms, r.a, r.b));
    *nq = r.nq; *h = r.h; *ci = r.ci;
    return WS_OK;
}

int ws_timer_read_layer(int32_t i, float* ms)
{
    WS_REQUIRE(i >= 0 && i < (int)timer_recs().size() && ms, "bad timer record index %d", i);
    const TimerRec& r = timer_recs()[i];
    WS_HIP(hipEventSynchronize(r.c));
    WS_HIP(hipEventElapsedTime(ms, r.a, r.c));
    return WS_OK;
}

}  // extern "C"
