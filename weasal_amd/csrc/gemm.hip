// weasal_amd/csrc/gemm.hip -- tall-skinny fp32 GEMMs on the f32-input MFMA (v_mfma_f32_32x32x2_f32).
//
// The dense parts of the KPConv hot path are all "M huge, K and N small":
//   the per-point unary MLPs            y = x W^T            (models/blocks.py:490-501, nn.Linear)
//   the kernel contraction               out = wf [N,15Ci] x weights [15Ci,Co]   (blocks.py:370-374)
// and their autograd (dx = dy W, dW = dy^T x).  With M = 400 000 rows and N,K in 32..512 they are
// bound by streaming the tall operand once; rocBLAS's fp32 solutions for these shapes run at a
// few % of that (profiles/r01_*).  Two kernels cover everything:
//
//   gemm_xb  : Y[M,N]  = X[M,K] * B[K,N]        B row-major, small.  (forward and dX)       gemm_xb.hip
//   gemm_xty : O[K,N]  = X[M,K]^T * Y[M,N]      reduction over the tall dimension.  (dW)    gemm_xty.hip
//   (and the activation backward with the bias gradient's column sums, ws_act_bwd_colsum*:   gemm_colsum.hip)
//
// Both stage 32-deep tiles in LDS with coalesced 16-byte loads (register prefetch of the next
// tile under the MFMAs of the current one) and feed v_mfma_f32_32x32x2_f32: exact fp32 (one
// rounding per product, a k-ordered fma chain), so results differ from rocBLAS only by summation
// order.  A operand lane map: A[i = lane&31][k = lane>>5]; B: B[k = lane>>5][j = lane&31];
// C/D: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)  (cdna_hip_programming.md section 3).
//
// This file holds the C entries: checks, launch plans, the bucketing of grouped calls, reporters.  No kernel is launched from it:
// an entry validates, plans, and calls the launch_* function of the family unit (gemm_launch.h), then passes the launch check
// that counts it (a grouped gemm_xb2 launch passes its own, gemm_xb.hip).  Every selection rule is here.
#include "gemm_launch.h"

using namespace gemm;

extern "C" {
// diagnostic switches (not part of the drop-in surface of include/weasal_hip.h)
int ws_gemm_shallow = 1;     // products with k <= 64 that the MFMA tiles do not take (k % 32 != 0), n % 4 == 0, many rows: 1 = gemm_xb_shallow_kernel, 0 = gemm_xb_kernel
int ws_gemm_staged = 1;     // gemm_xb2 epilogue: 1 = the tile turned through LDS (whole 128-byte row segments per store), 0 = per-lane rows
}

namespace {

int64_t colsum_chunk(int64_t m)
{
    int64_t c = ws_ceil_div(m, 768);
    return c < 16 ? 16 : c;                             // <= 768 chunks (three workgroups per CU) of >= 16 rows
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// chunk sums -> out: the wide form for large outputs of few chunks, the grouped form otherwise
bool reduce_partials_wide(const void* partial, int64_t elems, int chunks, const void* out, int n, int64_t ldo)
{
    return elems >= 65536 && chunks <= 64 && elems % 4 == 0 && al16(partial) && al16(out) && (ldo <= n || (n % 4 == 0 && ldo % 4 == 0));
}

int64_t xty_chunk(int64_t m, int k, int n)
{
    if (m >= 32768) {
        // tall operands: <= 256 chunks, a multiple of BK rows each, at least 512 rows (keeps >= 256 workgroups in
        // flight even when K fits one k-tile)
        int64_t c = ws_ceil_div(m, 256);
        if (c < 512) c = 512;
        return ws_ceil_div(c, BK) * BK;
    }
    // short operands (the deep pyramid levels): one chunk is a serial chain of m / 2 MFMA steps per wave, so the rows are
    // split until the chain (A / chunks) balances the write + re-read of the partial outputs (B * chunks):
    //   A = m/2 steps x 4 tiles x 64 cycles at 2.4 GHz,  B = 2 x 4 k n bytes at ~2 TB/s (measured: scattered partial stores),  chunks = sqrt(A / B),
    // at most 256 workgroups (tiles of 128 x 128 outputs x chunks: one per CU -- beyond that the MFMA pipes are shared and
    // more chunks only add partial traffic; 257..511 workgroups would double the time) and at least 32 rows per chunk.
    const double a_us = (double)m * 0.5 * 4.0 * 64.0 / 2400.0;
    const double b_us = 16.0 * (double)k * (double)n / 4.0e6;
    const int64_t tiles = ws_ceil_div(k, 128) * ws_ceil_div(n, 128);
    int64_t chunks = (int64_t)(__builtin_sqrt(a_us / b_us) + 0.5);
    if (chunks > 256 / tiles) chunks = 256 / tiles;
    if (chunks > m / 32) chunks = m / 32;
    if (chunks < 1) chunks = 1;
    return ws_ceil_div(ws_ceil_div(m, chunks), BK) * BK;
}

constexpr int THIN_K = 64;    // products with k <= this take 64-column tiles (more, lighter workgroups: they are all prologue and epilogue) instead of 128

// ---------------------------------------------------------------------------------------------
// A product travels as a record -- ws_xb_problem / ws_xty_problem (ws_common.h) -- that every entry, single or grouped, fills.
// Per family: one validator (its messages carry "member <i>: " in a group), one plan shared with the reporter, one run; and in
// the family unit one launcher per kernel that dispatches the plan onto the template arguments (ws_dispatch.h).
// ---------------------------------------------------------------------------------------------

// a failed requirement of a product: the message of the single entries (member < 0), behind "member <i>: " for a group's member i
int product_fail(int member, int code, const char* fmt, ...)
{
    char* buf = ws_errbuf();
    const int off = member >= 0 ? snprintf(buf, 512, "member %d: ", member) : 0;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf + off, 512 - (size_t)off, fmt, ap);
    va_end(ap);
    return code;
}
#define PRODUCT_REQUIRE(member, cond, ...) do { if (!(cond)) return product_fail(member, WS_ERR_INVALID, __VA_ARGS__); } while (0)

// ---- gemm_xb ----------------------------------------------------------------------------------------------------------------
int xb_validate(const ws_xb_problem& q, int member)
{
    PRODUCT_REQUIRE(member, q.m >= 0 && q.k >= 1 && q.n >= 1 && q.ldx >= q.k && q.ldy >= q.n, "bad sizes m=%lld k=%d n=%d", (long long)q.m, q.k, q.n);
    PRODUCT_REQUIRE(member, !q.residual || q.ldr >= q.n, "residual leading dimension too small");
    PRODUCT_REQUIRE(member, q.act == 0 || q.act == 1, "unknown activation %d", q.act);
    PRODUCT_REQUIRE(member, q.drop_p >= 0.0f && q.drop_p < 1.0f, "bad drop probability %g", (double)q.drop_p);
    PRODUCT_REQUIRE(member, !q.res_rows || (q.residual && q.res_rows_ld >= 1 && q.res_nrows >= 0), "gathered residual: NULL residual / bad sizes");
    PRODUCT_REQUIRE(member, !q.gate_y || q.ldg >= q.n, "gate leading dimension too small");
    PRODUCT_REQUIRE(member, !q.mask || q.ldm >= q.n, "mask leading dimension too small");
    PRODUCT_REQUIRE(member, q.m == 0 || (q.x && q.b && q.y), "NULL argument");
    return WS_OK;
}

// The launch a product takes (XbPlan, gemm_launch.h): every selection rule of the xb entries, shared with the reporter
// ws_gemm_xb_variant (which only reads the pointers' alignment).
int xb_plan(const ws_xb_problem& q, XbPlan& p)
{
    p = XbPlan{};
    if (q.m == 0) return WS_OK;
    const int64_t m = q.m, brs = xb_brs(q), bcs = q.b_col_stride;
    const int k = q.k, n = q.n;
    const int vecx = al16(q.x) && (q.ldx % 4 == 0);
    const int vecb = al16(q.b) && (n % 4 == 0);
    const int64_t gx = ws_ceil_div(m, BM);
    WS_REQUIRE(gx < (1ll << 31), "m too large");
    // what the float4 epilogues ask of everything they touch
    const bool epi4 = n % 4 == 0 && al16(q.y) && q.ldy % 4 == 0 && (!q.residual || (al16(q.residual) && q.ldr % 4 == 0)) &&
                      (!q.bias || al16(q.bias)) && (!q.gate_y || (al16(q.gate_y) && q.ldg % 4 == 0)) &&
                      (!q.mask || ((reinterpret_cast<uintptr_t>(q.mask) & 3u) == 0 && q.ldm % 4 == 0));
    if (vecx && k % 32 == 0 && epi4 && (int64_t)(k - 1) * brs + (int64_t)(n - 1) * bcs < (1ll << 29) && 128 * q.ldx < (1ll << 29) &&
        al16(q.b) && (bcs == 1 ? true : (brs == 1 && bcs % 4 == 0))) {
        const int64_t tiles = ws_ceil_div(m, 32);
        int wn = tiles >= 2048 ? 1 : 2;
        if (n <= 32) wn = 1;
        const int nt = wn == 1 ? (n <= 32 ? 1 : (n <= 64 || k <= THIN_K) ? 2 : 4) : (n <= 64 ? 1 : 2);
        const unsigned gx2 = (unsigned)ws_ceil_div(m, 32 * (4 / wn)), gy2 = (unsigned)ws_ceil_div(n, 32 * nt * wn);
        const int nch = k / 32;
        int splits = 1;
        if (q.scratch && (int64_t)gx2 * gy2 < 256 && nch >= 16) {
            splits = (int)ws_ceil_div(768, (int64_t)gx2 * gy2);
            if (splits > nch / 8) splits = nch / 8;
            if (splits > 16) splits = 16;
            if ((int64_t)splits * m * n * 4 > q.scratch_bytes) splits = (int)(q.scratch_bytes / (m * n * 4));
            if (splits < 2) splits = 1;
        }
        const int csplit = (int)ws_ceil_div(nch, splits);
        splits = (int)ws_ceil_div(nch, csplit);
        p.kind = XB_XB2; p.nt = nt; p.wn = wn; p.grid = dim3(gx2, gy2, (unsigned)splits);
        p.splits = splits; p.csplit = csplit; p.staged = ws_gemm_staged;
        return WS_OK;
    }
    WS_REQUIRE(bcs == 1 && brs == n, "a strided small matrix needs k %% 32 == 0, n %% 4 == 0 and 16-byte aligned rows "
                                     "(k=%d n=%d): pass a row-major [K,N] copy for this shape", k, n);
    if (ws_gemm_shallow && k <= 64 && n <= 1024 && (int64_t)k * n <= 8192 && m >= 4096 && al16(q.b) && epi4) {
        // shallow, ragged contraction over many rows: the streaming VALU form (gemm_xb_shallow_kernel)
        const int per = 256 / (n / 4);
        const int kp = (k + 3) & ~3;
        p.kind = XB_SHALLOW;
        p.rows = per * 8;                                               // 8 row passes per workgroup
        p.grid = dim3((unsigned)ws_ceil_div(m, p.rows));
        p.lds = sizeof(float) * ((size_t)kp * n + (size_t)p.rows * kp);
        return WS_OK;
    }
    p.kind = XB_GENERIC; p.vecx = vecx; p.vecb = vecb;
    // measured (tools/gemm_bench.py, M = 400k): for n > 64, shallow K is latency bound and prefers the 64-column
    // tile (more waves per SIMD, L2 serves the X re-read); deep K prefers the 128-column tile (X reuse)
    p.nt = n <= 32 ? 1 : (n <= 64 || k < 128) ? 2 : 4;
    p.grid = dim3((unsigned)gx, n <= 64 ? 1u : (unsigned)ws_ceil_div(n, 32 * p.nt));
    return WS_OK;
}

// product q (m > 0) by its plan: ONE counted launch (the epilogue of a split product counts with it: ws_common.h)
int xb_launch(const ws_xb_problem& q, const XbPlan& p, hipStream_t st)
{
    int rc = WS_OK;
    if (p.kind == XB_XB2) {
        rc = launch_xb2(q, p, st);
        if (rc == WS_OK && p.splits > 1) launch_splitk_epilogue(q, p, st);
    } else if (p.kind == XB_SHALLOW) {
        launch_xb_shallow(q, p, st);
    } else {
        rc = launch_xb_generic(q, p, st);
    }
    if (rc != WS_OK) return rc;
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int xb_run(const ws_xb_problem& q, void* stream)
{
    int rc = xb_validate(q, -1);
    if (rc != WS_OK || q.m == 0) return rc;
    XbPlan p;
    rc = xb_plan(q, p);
    return rc != WS_OK ? rc : xb_launch(q, p, (hipStream_t)stream);
}

// the record of the plain product y = x b, b row-major [K, N]: the entries add their strides, epilogue and gates
ws_xb_problem xb_problem(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int32_t n, float* y, int64_t ldy,
                         void* scratch = nullptr, int64_t scratch_bytes = 0)
{
    ws_xb_problem q{};
    q.x = x; q.m = m; q.k = k; q.ldx = ldx;
    q.b = b; q.b_row_stride = -1; q.b_col_stride = 1; q.n = n;
    q.y = y; q.ldy = ldy;
    q.scratch = scratch; q.scratch_bytes = scratch_bytes;
    return q;
}
void xb_epilogue(ws_xb_problem& q, const float* bias, const float* residual, int64_t ldr, int32_t act, float slope)
{
    q.bias = bias; q.residual = residual; q.ldr = ldr; q.act = act; q.slope = slope;
}
void xb_strides(ws_xb_problem& q, int64_t b_row_stride, int64_t b_col_stride)
{
    q.b_row_stride = b_row_stride; q.b_col_stride = b_col_stride;
}

// ---- grouped products (ws_common.h) ------------------------------------------------------------------------------------------
// Each member keeps exactly the plan it gets alone from xb_plan / xty_plan -- kind, tile variant, splits, csplit, chunk,
// chunks, reduction form, pitched output -- and its workgroups run the single kernels' bodies on that plan, so every sum
// is added in the order of the single launch: a grouped result is bit-identical to the single one.  Only the number of
// launches changes.
// one call plans at most GROUP_CALL_MAX members on the stack (no allocation on the launch path: the block calls pass 2 .. 4);
// a longer list is handled as consecutive slices of that many, each grouped within itself
constexpr int GROUP_CALL_MAX = 16;
struct IdList {
    int n = 0;
    int v[GROUP_CALL_MAX];
    void push_back(int i) { v[n++] = i; }
    int size() const { return n; }
};
constexpr int64_t GROUP_MEMBER_BLOCKS = 1ll << 27;      // a member with more workgroups runs alone (the linear index stays 32-bit)

// the members of one instantiation, GROUP_MAX at a time (more spill into further launches): f(ids, cnt) -> WS_OK or the error
template <typename F>
int for_each_launch(const IdList& ids, F&& f)
{
    for (int off = 0; off < ids.size(); off += GROUP_MAX) {
        const int rc = f(ids.v + off, ids.size() - off < GROUP_MAX ? ids.size() - off : GROUP_MAX);
        if (rc != WS_OK) return rc;
    }
    return WS_OK;
}

// ---- gemm_xty -----------------------------------------------------------------------------------------------------------------
// bf16 rows (ws_gemm_xty_bf16) travel in the same record, x and y pointing at 2-byte elements: the row type is the `bf16` beside it
int xty_validate(const ws_xty_problem& q, int member)
{
    PRODUCT_REQUIRE(member, q.m >= 0 && q.k >= 1 && q.n >= 1 && q.ldx >= q.k && q.ldy >= q.n, "bad sizes m=%lld k=%d n=%d", (long long)q.m, q.k, q.n);
    PRODUCT_REQUIRE(member, q.out, "NULL argument");
    PRODUCT_REQUIRE(member, q.ldo == 0 || q.ldo >= q.n, "output pitch smaller than a row");
    PRODUCT_REQUIRE(member, q.m == 0 || (q.x && q.y && q.scratch), "NULL argument");
    return WS_OK;
}

// The launches of a dW reduction (XtyPlan, gemm_launch.h): every selection rule of the xty entries, shared with the reporter
// ws_gemm_xty_variant (which only reads the pointers' alignment).  bf16: 2-byte operands (no gemm_xty_kernel fallback).
int xty_plan(const ws_xty_problem& q, bool bf16, XtyPlan& p)
{
    p = XtyPlan{};
    p.bf16 = bf16;
    p.pitched = q.ldo > q.n;
    if (q.m == 0) return WS_OK;
    const int k = q.k, n = q.n;
    p.chunk = xty_chunk(q.m, k, n);
    p.chunks = (int)ws_ceil_div(q.m, p.chunk);
    const int64_t span = p.chunk * (q.ldx > q.ldy ? q.ldx : q.ldy);
    if (bf16) WS_REQUIRE(span * 2 < (1ll << 31), "operand exceeds the 32-bit buffer offsets");
    p.partial = (p.chunks == 1 && !p.pitched) ? q.out : (float*)q.scratch;
    p.lds = !bf16 && span * 4 >= (1ll << 31);
    if (!p.lds) {
        // per-wave tile (32 KT) x (32 NT); waves WK x WN over the output, the rest split the rows
        const bool a2x = bf16 ? (reinterpret_cast<uintptr_t>(q.x) & 3u) == 0 && q.ldx % 2 == 0 && k % 2 == 0
                              : (reinterpret_cast<uintptr_t>(q.x) & 7u) == 0 && q.ldx % 2 == 0;
        const bool a2y = bf16 ? (reinterpret_cast<uintptr_t>(q.y) & 3u) == 0 && q.ldy % 2 == 0 && n % 2 == 0
                              : (reinterpret_cast<uintptr_t>(q.y) & 7u) == 0 && q.ldy % 2 == 0;
        p.kt = (k > 32 && a2x) ? 2 : 1;
        p.nt = (n > 32 && a2y) ? 2 : 1;
        p.wk = k > 32 * p.kt ? 2 : 1;
        p.wn = (n > 32 * p.nt && p.wk == 1) || (n > 32 * p.nt && k > 32 * p.kt) ? 2 : 1;
        p.grid = dim3(p.chunks, (unsigned)ws_ceil_div(k, 32 * p.kt * p.wk), (unsigned)ws_ceil_div(n, 32 * p.nt * p.wn));
    } else {
        p.vecx = al16(q.x) && (q.ldx % 4 == 0);
        p.vecy = al16(q.y) && (q.ldy % 4 == 0);
        p.kt = k <= 32 ? 1 : (k <= 64 ? 2 : 4);
        p.nt = n <= 32 ? 1 : (n <= 64 ? 2 : 4);
        p.grid = dim3(p.chunks, (unsigned)ws_ceil_div(k, 32 * p.kt), (unsigned)ws_ceil_div(n, 32 * p.nt));
    }
    if (p.chunks > 1 || p.pitched)
        p.reduce = reduce_partials_wide(p.partial, (int64_t)k * n, p.chunks, q.out, n, p.pitched ? q.ldo : 0) ? 2 : 1;
    return WS_OK;
}

// the product launch of plan p: counted
int xty_product_launch(const ws_xty_problem& q, const XtyPlan& p, hipStream_t st)
{
    const int rc = p.lds ? launch_xty_lds(q, p, st) : launch_xty2(q, p, st);
    if (rc != WS_OK) return rc;
    WS_LAUNCH_CHECK();
    return WS_OK;
}
// the chunk sums of plan p (p.reduce != 0): counted
int xty_reduce_launch(const ws_xty_problem& q, const XtyPlan& p, hipStream_t st)
{
    launch_reduce_partials(p.reduce == 2, p.partial, (int64_t)q.k * q.n, p.chunks, q.out, st, q.n, p.pitched ? q.ldo : 0);
    WS_LAUNCH_CHECK();
    return WS_OK;
}
// the grouped forms of the two (members id[0 .. cnt) of one instantiation; the chunk sums of cnt members): counted, one each
int xty_group_launch(const ws_xty_problem* q, const XtyPlan* plan, const int* id, int cnt, hipStream_t st)
{
    const int rc = launch_xty2_group(q, plan, id, cnt, st);
    if (rc != WS_OK) return rc;
    WS_LAUNCH_CHECK();
    return WS_OK;
}
int xty_reduce_group_launch(const ws_xty_problem* q, const XtyPlan* plan, const int* id, int cnt, hipStream_t st)
{
    launch_reduce_group(q, plan, id, cnt, st);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int xty_run(const ws_xty_problem& q, bool bf16, void* stream)
{
    int rc = xty_validate(q, -1);
    if (rc != WS_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (q.m == 0) {
        if (q.ldo > q.n) WS_HIP(hipMemset2DAsync(q.out, sizeof(float) * (size_t)q.ldo, 0, sizeof(float) * (size_t)q.n, (size_t)q.k, st));
        else WS_HIP(hipMemsetAsync(q.out, 0, sizeof(float) * (size_t)q.k * q.n, st));
        return WS_OK;
    }
    XtyPlan p;
    rc = xty_plan(q, bf16, p);
    if (rc == WS_OK) rc = xty_product_launch(q, p, st);
    if (rc == WS_OK && p.reduce) rc = xty_reduce_launch(q, p, st);
    return rc;
}

const char* reduce_name(int r)
{
    return r == 2 ? "reduce_partials_wide_kernel" : (r == 1 ? "reduce_partials_kernel" : "none");
}

}  // namespace

extern "C" {

int64_t ws_gemm_xb_scratch_bytes(int64_t m, int32_t k, int32_t n)
{
    // room for up to 16 split-K partial outputs; only short, deep products use it
    if (m <= 0 || m >= 32768 || k < 512) return 0;
    return 16 * m * (int64_t)n * (int64_t)sizeof(float);
}

int ws_gemm_xb(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int32_t n, float* y, int64_t ldy,
               void* stream)
{
    return xb_run(xb_problem(x, m, k, ldx, b, n, y, ldy), stream);
}

int ws_gemm_xb_epilogue(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int32_t n,
                        const float* bias, const float* residual, int64_t ldr, int32_t act, float slope,
                        float* y, int64_t ldy, void* stream)
{
    ws_xb_problem q = xb_problem(x, m, k, ldx, b, n, y, ldy);
    xb_epilogue(q, bias, residual, ldr, act, slope);
    return xb_run(q, stream);
}

int ws_gemm_xb_epilogue_splitk(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int32_t n,
                               const float* bias, const float* residual, int64_t ldr, int32_t act, float slope,
                               float* y, int64_t ldy, void* scratch, int64_t scratch_bytes, void* stream)
{
    ws_xb_problem q = xb_problem(x, m, k, ldx, b, n, y, ldy, scratch, scratch_bytes);
    xb_epilogue(q, bias, residual, ldr, act, slope);
    return xb_run(q, stream);
}

int ws_gemm_xb_epilogue_strided(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int64_t b_row_stride,
                                int64_t b_col_stride, int32_t n, const float* bias, const float* residual, int64_t ldr,
                                int32_t act, float slope, float* y, int64_t ldy, void* scratch, int64_t scratch_bytes,
                                void* stream)
{
    ws_xb_problem q = xb_problem(x, m, k, ldx, b, n, y, ldy, scratch, scratch_bytes);
    xb_strides(q, b_row_stride, b_col_stride);
    xb_epilogue(q, bias, residual, ldr, act, slope);
    return xb_run(q, stream);
}

int ws_gemm_xb_gated_strided(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int64_t b_row_stride,
                             int64_t b_col_stride, int32_t n, const float* bias, const float* residual, int64_t ldr,
                             int32_t act, float slope, const float* gate_y, int64_t ldg, float gate_slope, const uint8_t* mask,
                             int64_t ldm, float mask_scale, float* y, int64_t ldy, void* scratch, int64_t scratch_bytes,
                             void* stream)
{
    ws_xb_problem q = xb_problem(x, m, k, ldx, b, n, y, ldy, scratch, scratch_bytes);
    xb_strides(q, b_row_stride, b_col_stride);
    xb_epilogue(q, bias, residual, ldr, act, slope);
    q.gate_y = gate_y; q.ldg = ldg; q.gate_slope = gate_slope;
    q.mask = mask; q.ldm = ldm; q.mask_scale = mask_scale;
    return xb_run(q, stream);
}

int ws_gemm_xb_dropout_strided(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int64_t b_row_stride,
                               int64_t b_col_stride, int32_t n, const float* bias, const float* residual, int64_t ldr,
                               int32_t act, float slope, float drop_p, uint64_t drop_seed, float* y, int64_t ldy, void* scratch,
                               int64_t scratch_bytes, void* stream)
{
    ws_xb_problem q = xb_problem(x, m, k, ldx, b, n, y, ldy, scratch, scratch_bytes);
    xb_strides(q, b_row_stride, b_col_stride);
    xb_epilogue(q, bias, residual, ldr, act, slope);
    q.drop_p = drop_p; q.drop_seed = drop_seed;
    return xb_run(q, stream);
}

int ws_gemm_xb_gate_dropout(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int32_t n, const float* gate_y,
                            int64_t ldg, float gate_slope, float drop_p, uint64_t drop_seed, float* y, int64_t ldy, void* scratch,
                            int64_t scratch_bytes, void* stream)
{
    ws_xb_problem q = xb_problem(x, m, k, ldx, b, n, y, ldy, scratch, scratch_bytes);
    q.gate_y = gate_y; q.ldg = ldg; q.gate_slope = gate_slope;
    q.drop_p = drop_p; q.drop_seed = drop_seed;
    return xb_run(q, stream);
}

// private to the library (ws_common.h): the strided product with the whole epilogue menu -- dropout (drop_p > 0) and / or a
// gathered residual (res_rows != NULL: row r adds residual[res_rows[r * res_rows_ld]], indices outside [0, res_nrows) add nothing)
int ws_priv_gemm_xb_ex(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int64_t b_row_stride, int64_t b_col_stride,
                       int32_t n, const float* bias, const float* residual, int64_t ldr, const int64_t* res_rows, int64_t res_rows_ld,
                       int64_t res_nrows, int32_t act, float slope, float drop_p, uint64_t drop_seed, float* y, int64_t ldy,
                       void* scratch, int64_t scratch_bytes, void* stream)
{
    ws_xb_problem q = xb_problem(x, m, k, ldx, b, n, y, ldy, scratch, scratch_bytes);
    xb_strides(q, b_row_stride, b_col_stride);
    xb_epilogue(q, bias, residual, ldr, act, slope);
    q.res_rows = res_rows; q.res_rows_ld = res_rows_ld; q.res_nrows = res_nrows;
    q.drop_p = drop_p; q.drop_seed = drop_seed;
    return xb_run(q, stream);
}

// private to the library (ws_common.h).  Members whose plan is not gemm_xb2 (the shallow and generic forms) run alone, as do
// members alone in their instantiation; m == 0 does what the single entry does (nothing); more than GROUP_MAX members of one
// instantiation spill into a second launch.
int ws_priv_gemm_xb_group(const ws_xb_problem* q, int32_t count, void* stream)
{
    WS_REQUIRE(count >= 0 && (q || count == 0), "bad group");
    for (; count > GROUP_CALL_MAX; q += GROUP_CALL_MAX, count -= GROUP_CALL_MAX) {
        const int rc = ws_priv_gemm_xb_group(q, GROUP_CALL_MAX, stream);
        if (rc != WS_OK) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    XbPlan plan[GROUP_CALL_MAX];
    IdList bucket[XB2_NPAIRS];
    for (int i = 0; i < count; ++i) {
        int rc = xb_validate(q[i], i);
        if (rc != WS_OK) return rc;
        if (q[i].m == 0) continue;
        const XbPlan& p = plan[i];
        rc = xb_plan(q[i], plan[i]);
        if (rc != WS_OK) return rc;
        if (p.kind != XB_XB2 || (int64_t)p.grid.x * p.grid.y * p.grid.z >= GROUP_MEMBER_BLOCKS) {
            rc = xb_launch(q[i], p, st);
            if (rc != WS_OK) return rc;
            continue;
        }
        if (xb2_pair(p.nt, p.wn) < 0) return xb2_no_instantiation(p);
        bucket[xb2_pair(p.nt, p.wn)].push_back(i);
    }
    for (const IdList& ids : bucket) {
        const int rc = for_each_launch(ids, [&](const int* id, int cnt) {
            return cnt == 1 ? xb_launch(q[id[0]], plan[id[0]], st) : launch_xb2_group(q, plan, id, cnt, st);
        });
        if (rc != WS_OK) return rc;
    }
    return WS_OK;
}

int64_t ws_act_bwd_colsum_scratch_bytes(int64_t m, int32_t n)
{
    return ws_ceil_div(m > 0 ? m : 1, colsum_chunk(m)) * (int64_t)n * (int64_t)sizeof(float);
}

// The launches of act_bwd_colsum_impl (m > 0; ColsumPlan, gemm_launch.h), shared with the reporter ws_act_bwd_colsum_variant
static ColsumPlan colsum_plan(const void* dy, int64_t m, int32_t n, int64_t lddy, const void* y, int64_t ldy, const void* dz,
                              int64_t lddz, float* colsum, void* scratch)
{
    ColsumPlan p{};
    p.chunk = colsum_chunk(m);
    p.chunks = (int)ws_ceil_div(m, p.chunk);
    p.partial = colsum ? (p.chunks == 1 ? colsum : (float*)scratch) : nullptr;
    p.reduce = colsum && p.chunks > 1;
    const bool vec = n % 4 == 0 && al16(dy) && lddy % 4 == 0 && (!y || (al16(y) && ldy % 4 == 0 && al16(dz) && lddz % 4 == 0));
    p.v = vec ? 4 : 1;
    p.grid = dim3(p.chunks, (unsigned)ws_ceil_div(ws_ceil_div(n, p.v), 256));
    return p;
}

static int act_bwd_colsum_impl(const float* dy, int64_t m, int32_t n, int64_t lddy, const float* y, int64_t ldy, float slope,
                               float* dz, int64_t lddz, float* colsum, void* scratch, void* stream, WsDrop drop)
{
    WS_REQUIRE(m >= 0 && n >= 1 && lddy >= n, "bad sizes m=%lld n=%d", (long long)m, n);
    WS_REQUIRE(!y || (dz && ldy >= n && lddz >= n), "activation backward needs y and dz");
    WS_REQUIRE(!colsum || scratch, "column sums need scratch");
    hipStream_t st = (hipStream_t)stream;
    if (m == 0) {
        if (colsum) WS_HIP(hipMemsetAsync(colsum, 0, sizeof(float) * (size_t)n, st));
        return WS_OK;
    }
    WS_REQUIRE(dy && (y || colsum), "NULL argument");
    const ColsumPlan p = colsum_plan(dy, m, n, lddy, y, ldy, dz, lddz, colsum, scratch);
    const int rc = launch_act_bwd_colsum(p, dy, m, n, lddy, y, ldy, slope, dz, lddz, drop, st);
    if (rc != WS_OK) return rc;
    WS_LAUNCH_CHECK();
    if (p.reduce) {
        launch_reduce_partials(false, p.partial, n, p.chunks, colsum, st);
        WS_LAUNCH_CHECK();
    }
    return WS_OK;
}

int ws_act_bwd_colsum(const float* dy, int64_t m, int32_t n, int64_t lddy, const float* y, int64_t ldy, float slope,
                      float* dz, int64_t lddz, float* colsum, void* scratch, void* stream)
{
    return act_bwd_colsum_impl(dy, m, n, lddy, y, ldy, slope, dz, lddz, colsum, scratch, stream, WsDrop{});
}

int ws_act_bwd_colsum_dropout(const float* dy, int64_t m, int32_t n, int64_t lddy, const float* y, int64_t ldy, float slope,
                              float drop_p, uint64_t drop_seed, float* dz, int64_t lddz, float* colsum, void* scratch, void* stream)
{
    WS_REQUIRE(drop_p >= 0.0f && drop_p < 1.0f, "bad drop probability %g", (double)drop_p);
    WS_REQUIRE(y && dz, "the dropout form writes dz (it needs y and dz)");
    return act_bwd_colsum_impl(dy, m, n, lddy, y, ldy, slope, dz, lddz, colsum, scratch, stream, ws_drop_args(drop_p, drop_seed));
}

int64_t ws_gemm_xty_scratch_bytes(int64_t m, int32_t k, int32_t n)
{
    // (xty_chunk(0, ..) is 0: size an empty operand as one row, like ws_act_bwd_colsum_scratch_bytes)
    const int64_t rows = m > 0 ? m : 1;
    return ws_ceil_div(rows, xty_chunk(rows, k, n)) * (int64_t)k * n * (int64_t)sizeof(float);
}

int ws_gemm_xty(const float* x, int64_t m, int32_t k, int64_t ldx, const float* y, int32_t n, int64_t ldy,
                float* out, void* scratch, void* stream)
{
    return xty_run(ws_xty_problem{x, m, k, ldx, y, n, ldy, out, 0, scratch, 0}, false, stream);
}

// dW = X^T dY with bf16 rows (BASELINE config 5): the LDS-free reduction with 2-byte operand loads; no pitched form.
// Requirements: k, n even or <= 32 handled by the one-column form; every shape of the bf16 path qualifies.
int ws_gemm_xty_bf16(const uint16_t* x, int64_t m, int32_t k, int64_t ldx, const uint16_t* y, int32_t n, int64_t ldy,
                     float* out, void* scratch, void* stream)
{
    return xty_run(ws_xty_problem{(const float*)x, m, k, ldx, (const float*)y, n, ldy, out, 0, scratch, 0}, true, stream);
}

// private to the library (ws_common.h): dW written as a column block of a wider matrix (row pitch ldo >= n)
int ws_priv_gemm_xty_pitched(const float* x, int64_t m, int32_t k, int64_t ldx, const float* y, int32_t n, int64_t ldy, float* out,
                             int64_t ldo, void* scratch, void* stream)
{
    WS_REQUIRE(ldo >= n, "output pitch smaller than a row");      // (this entry has no ldo = 0: the record's flat form)
    return xty_run(ws_xty_problem{x, m, k, ldx, y, n, ldy, out, ldo, scratch, 0}, false, stream);
}

// private to the library (ws_common.h).  Members in the 32-bit-overflow form (gemm_xty_kernel) run alone, reduction
// included; m == 0 clears the output like the single entry.  The others launch their products grouped by instantiation
// (alone when nobody shares it; more than GROUP_MAX spill into a second launch), then the chunk sums of all of them are
// added by grouped reduction launches of up to GROUP_MAX members.
int ws_priv_gemm_xty_group(const ws_xty_problem* q, int32_t count, void* stream)
{
    WS_REQUIRE(count >= 0 && (q || count == 0), "bad group");
    for (; count > GROUP_CALL_MAX; q += GROUP_CALL_MAX, count -= GROUP_CALL_MAX) {
        const int rc = ws_priv_gemm_xty_group(q, GROUP_CALL_MAX, stream);
        if (rc != WS_OK) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    XtyPlan plan[GROUP_CALL_MAX];
    IdList bucket[16], red;
    for (int i = 0; i < count; ++i) {
        const ws_xty_problem& a = q[i];
        int rc = xty_validate(a, i);
        if (rc != WS_OK) return rc;
        if (a.m > 0 && a.scratch_bytes < ws_gemm_xty_scratch_bytes(a.m, a.k, a.n))
            return product_fail(i, WS_ERR_CAPACITY, "scratch too small: %lld < %lld bytes", (long long)a.scratch_bytes,
                                (long long)ws_gemm_xty_scratch_bytes(a.m, a.k, a.n));
        const XtyPlan& p = plan[i];
        rc = xty_plan(a, false, plan[i]);
        if (rc != WS_OK) return rc;
        if (a.m == 0 || p.lds || (int64_t)p.grid.x * p.grid.y * p.grid.z >= GROUP_MEMBER_BLOCKS) {
            rc = xty_run(a, false, stream);
            if (rc != WS_OK) return rc;
            continue;
        }
        bucket[(((p.kt - 1) * 2 + (p.nt - 1)) * 2 + (p.wk - 1)) * 2 + (p.wn - 1)].push_back(i);
        if (p.reduce) red.push_back(i);
    }
    for (const IdList& ids : bucket) {
        const int rc = for_each_launch(ids, [&](const int* id, int cnt) {
            return cnt == 1 ? xty_product_launch(q[id[0]], plan[id[0]], st) : xty_group_launch(q, plan, id, cnt, st);
        });
        if (rc != WS_OK) return rc;
    }
    return for_each_launch(red, [&](const int* id, int cnt) {
        return cnt == 1 ? xty_reduce_launch(q[id[0]], plan[id[0]], st) : xty_reduce_group_launch(q, plan, id, cnt, st);
    });
}

// ---------------------------------------------------------------------------------------------
// Reporters: the launches the entries above make for these arguments (the same validators and plan functions; pointers are
// only tested for NULL and alignment, nothing is read or launched).  Form: "kernel<template arguments> key=value ...".
// ---------------------------------------------------------------------------------------------
// ws_gemm_xb* / ws_priv_gemm_xb_ex: b_row_stride < 0 = row-major [K, N] (the non-strided entries); gate_y / mask as in
// ws_gemm_xb_gated_strided (dropout and the gathered residual do not change the launch)
int ws_gemm_xb_variant(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int64_t b_row_stride, int64_t b_col_stride,
                       int32_t n, const float* bias, const float* residual, int64_t ldr, const float* gate_y, int64_t ldg,
                       const uint8_t* mask, int64_t ldm, const float* y, int64_t ldy, const void* scratch, int64_t scratch_bytes,
                       char* out, int32_t cap)
{
    WS_REQUIRE(out && cap > 0, "bad argument");
    ws_xb_problem q = xb_problem(x, m, k, ldx, b, n, const_cast<float*>(y), ldy, const_cast<void*>(scratch), scratch_bytes);
    xb_strides(q, b_row_stride, b_col_stride);
    q.bias = bias; q.residual = residual; q.ldr = ldr;
    q.gate_y = gate_y; q.ldg = ldg; q.mask = mask; q.ldm = ldm;
    XbPlan p;
    int rc = xb_validate(q, -1);
    if (rc == WS_OK) rc = xb_plan(q, p);
    if (rc != WS_OK) return rc;
    if (p.kind == XB_NONE)
        snprintf(out, (size_t)cap, "none (m == 0)");
    else if (p.kind == XB_XB2)
        snprintf(out, (size_t)cap, "gemm_xb2_kernel<NT=%d, WN=%d> b=%s epilogue=%s splits=%d csplit=%d%s", p.nt, p.wn,
                 xb_brs(q) == 1 ? "transposed" : "rows", p.staged ? "staged" : "lanes", p.splits, p.csplit,
                 p.splits > 1 ? " + splitk_epilogue_kernel" : "");
    else if (p.kind == XB_SHALLOW)
        snprintf(out, (size_t)cap, "gemm_xb_shallow_kernel rows=%d", p.rows);
    else
        snprintf(out, (size_t)cap, "gemm_xb_kernel<NT=%d, BKX=32> vecx=%d vecb=%d", p.nt, p.vecx, p.vecb);
    return WS_OK;
}

// ws_gemm_xty (ldo = 0), ws_priv_gemm_xty_pitched (ldo >= n) and, rows_bf16 = 1, ws_gemm_xty_bf16 (uint16_t rows, ldo = 0)
int ws_gemm_xty_variant(const void* x, int64_t m, int32_t k, int64_t ldx, const void* y, int32_t n, int64_t ldy, float* out_m,
                        int64_t ldo, void* scratch, int32_t rows_bf16, char* out, int32_t cap)
{
    WS_REQUIRE(out && cap > 0, "bad argument");
    WS_REQUIRE(!rows_bf16 || ldo == 0, "the bf16 reduction has no pitched form");
    const ws_xty_problem q{(const float*)x, m, k, ldx, (const float*)y, n, ldy, out_m, ldo, scratch, 0};
    XtyPlan p;
    int rc = xty_validate(q, -1);
    if (rc == WS_OK) rc = xty_plan(q, rows_bf16 != 0, p);
    if (rc != WS_OK) return rc;
    const char* form = p.pitched ? "pitched" : "flat";
    if (m == 0)
        snprintf(out, (size_t)cap, "memset (m == 0) out=%s", form);
    else if (!p.lds)
        snprintf(out, (size_t)cap, "gemm_xty2_kernel<KT=%d, NT=%d, WK=%d, WN=%d, TI=%s> chunk=%lld chunks=%d reduce=%s out=%s", p.kt, p.nt,
                 p.wk, p.wn, rows_bf16 ? "bf16" : "float", (long long)p.chunk, p.chunks, reduce_name(p.reduce), form);
    else
        snprintf(out, (size_t)cap, "gemm_xty_kernel<NT=%d, KT=%d> vecx=%d vecy=%d chunk=%lld chunks=%d reduce=%s out=%s", p.nt, p.kt,
                 p.vecx, p.vecy, (long long)p.chunk, p.chunks, reduce_name(p.reduce), form);
    return WS_OK;
}

// ws_act_bwd_colsum / ws_act_bwd_colsum_dropout (the dropout form launches the same kernels)
int ws_act_bwd_colsum_variant(const float* dy, int64_t m, int32_t n, int64_t lddy, const float* y, int64_t ldy, const float* dz,
                              int64_t lddz, float* colsum, void* scratch, char* out, int32_t cap)
{
    WS_REQUIRE(out && cap > 0, "bad argument");
    WS_REQUIRE(m >= 0 && n >= 1 && lddy >= n, "bad sizes m=%lld n=%d", (long long)m, n);
    if (m == 0) {
        snprintf(out, (size_t)cap, "%s (m == 0)", colsum ? "memset" : "none");
        return WS_OK;
    }
    const ColsumPlan p = colsum_plan(dy, m, n, lddy, y, ldy, dz, lddz, colsum, scratch);
    snprintf(out, (size_t)cap, "act_bwd_colsum_kernel<V=%d> chunk=%lld chunks=%d reduce=%s", p.v, (long long)p.chunk, p.chunks,
             reduce_name(p.reduce));
    return WS_OK;
}

}  // extern "C"
