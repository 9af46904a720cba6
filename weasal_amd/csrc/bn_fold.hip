// weasal_amd/csrc/bn_fold.hip -- evaluation-mode batch normalisation folded into the product in front of it.
//
// With running statistics, BN after a product is an affine map per output channel, so it belongs in the weights:
//     rstd_c = 1 / sqrt(running_var_c + eps)     a_c = gamma_c * rstd_c     t_c = beta_c - running_mean_c * a_c
//     act(BN(x W^T) + residual) = act(x (a (.)rows W)^T + t + residual)
// which is the product(bias, residual, slope) form every GEMM / KPConv epilogue and every block call of this library takes.
//
//   ws_bn_fold_fwd      bn_fold_fwd_kernel: w_out = a * w, t_out = beta - mean * a for a TABLE of sites in one launch
//   ws_bn_fold_bwd      bn_fold_bwd_kernel: dw = a * dw_out, dbeta = dt_out, dgamma = rstd * (sum dw_out * w - mean * dt_out)
//   ws_bn_fold_variant  the reporter; fold_plan is the ONE plan function of the three entries
//
// A site is a weight seen as [outer, c, inner] with the BN channel on the middle axis (nn.Linear.weight [c, k]: outer 1,
// inner k; KPConv weights [K, Ci, Co]: outer K * Ci, inner 1).  The table travels in the kernel arguments (the idiom of
// optim.hip), WS_BN_FOLD_MAX sites per launch; workgroups are dealt to the sites by a prefix over their element counts.
// float32 throughout; compiled with -ffp-contract=off: sqrtf, the division, every product and every sum round on their own,
// so a float64 restatement predicts the result to a few units in the last place.  The backward sums run in an order fixed
// by the shapes: no float atomics, run-to-run bit-identical.
#include "ws_common.h"

namespace {

constexpr int FOLD_MAX = WS_BN_FOLD_MAX;
constexpr int FOLD_CHUNK = 4096;       // elements of a weight per workgroup
constexpr int FOLD_THREADS = 256;
constexpr int FOLD_ROW_CH = 4;         // row sums: channels per workgroup (one wave each)
constexpr int FOLD_TALL = 1024;        // column sums: from this many rows on the narrow tile (more workgroups)

struct FoldFwdArgs {
    const float* w[FOLD_MAX];
    const float* gamma[FOLD_MAX];
    const float* beta[FOLD_MAX];
    const float* mean[FOLD_MAX];
    const float* var[FOLD_MAX];
    float* w_out[FOLD_MAX];
    float* t_out[FOLD_MAX];
    float eps[FOLD_MAX];
    int c[FOLD_MAX], inner[FOLD_MAX], n[FOLD_MAX];
    int first_block[FOLD_MAX + 1];
    unsigned char vec[FOLD_MAX];
    int count;
};

struct FoldBwdArgs {
    const float* w[FOLD_MAX];
    const float* gamma[FOLD_MAX];
    const float* mean[FOLD_MAX];
    const float* var[FOLD_MAX];
    const float* dw_out[FOLD_MAX];
    const float* dt_out[FOLD_MAX];
    float* dw[FOLD_MAX];
    float* dgamma[FOLD_MAX];
    float* dbeta[FOLD_MAX];
    float eps[FOLD_MAX];
    int c[FOLD_MAX], inner[FOLD_MAX], n[FOLD_MAX];
    int ew_blocks[FOLD_MAX];           // the site's first ew_blocks workgroups scale dw_out, the others sum for dgamma
    int first_block[FOLD_MAX + 1];
    unsigned char vec[FOLD_MAX], tile[FOLD_MAX];      // tile: 0 row sums, else columns per workgroup of the column sums
    int count;
};

// what one site takes: the ONE place where the branch is decided (launchers and reporter)
struct FoldPlan {
    int64_t n;          // elements of the weight
    int vec;            // 16-byte accesses in the element-wise part
    int ew_blocks;      // workgroups of the element-wise part
    int tile;           // backward: 0 row sums (a wave per channel), else columns per workgroup of the column sums
    int red_blocks;     // backward: workgroups of the dgamma sums
};

inline bool fold_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// src, dst: the [outer, c, inner] pointers the element-wise part reads and writes (w, w_out; backward dw_out, dw; NULL passes)
FoldPlan fold_plan(int64_t outer, int32_t c, int64_t inner, const void* src, const void* dst, bool backward, bool want_ew,
                   bool want_sums)
{
    FoldPlan p;
    p.n = outer * c * inner;
    // a quad of consecutive elements lies in one channel (inner % 4 == 0) or in four consecutive ones (inner == 1, c % 4 == 0)
    const bool shape_ok = inner % 4 == 0 || (inner == 1 && c % 4 == 0);
    p.vec = (shape_ok && fold_aligned(src) && fold_aligned(dst)) ? 1 : 0;
    p.ew_blocks = want_ew ? (int)ws_ceil_div(p.n, FOLD_CHUNK) : 0;
    p.tile = 0;
    p.red_blocks = 0;
    if (backward) {
        p.tile = inner == 1 ? (outer >= FOLD_TALL ? 16 : 64) : 0;
        if (want_sums) p.red_blocks = (int)ws_ceil_div(c, p.tile ? p.tile : FOLD_ROW_CH);
    }
    return p;
}

__device__ __forceinline__ int fold_site(const int* first_block, int count)
{
    // the prefix is ascending, <= WS_BN_FOLD_MAX entries: binary search on scalars
    int lo = 0, hi = count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first_block[mid] <= (int)blockIdx.x) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ float fold_rstd(float var, float eps) { return 1.0f / sqrtf(var + eps); }

// out[e] = a[channel of e] * src[e] over the chunk [base, end) of a site; src NULL = zeros
__device__ __forceinline__ void fold_scale_chunk(const float* __restrict__ src, float* __restrict__ out, const float* __restrict__ gamma,
                                                 const float* __restrict__ var, float eps, int c, int inner, int base, int end, int vec)
{
    if (vec) {
        for (int i = base + 4 * (int)threadIdx.x; i < end; i += 4 * FOLD_THREADS) {
            float4 v = src ? *reinterpret_cast<const float4*>(src + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (inner == 1) {
                const int ch = i % c;                          // c % 4 == 0 and i % 4 == 0: the quad stays inside the row
                v.x = (gamma[ch] * fold_rstd(var[ch], eps)) * v.x;             // ([c] vectors: any alignment)
                v.y = (gamma[ch + 1] * fold_rstd(var[ch + 1], eps)) * v.y;
                v.z = (gamma[ch + 2] * fold_rstd(var[ch + 2], eps)) * v.z;
                v.w = (gamma[ch + 3] * fold_rstd(var[ch + 3], eps)) * v.w;
            } else {
                const int ch = (i / inner) % c;                // inner % 4 == 0: one channel for the quad
                const float a = gamma[ch] * fold_rstd(var[ch], eps);
                v.x = a * v.x; v.y = a * v.y; v.z = a * v.z; v.w = a * v.w;
            }
            *reinterpret_cast<float4*>(out + i) = v;
        }
    } else {
        for (int e = base + (int)threadIdx.x; e < end; e += FOLD_THREADS) {
            const int ch = (e / inner) % c;
            const float a = gamma[ch] * fold_rstd(var[ch], eps);
            out[e] = a * (src ? src[e] : 0.0f);
        }
    }
}

__global__ __launch_bounds__(FOLD_THREADS) void bn_fold_fwd_kernel(const FoldFwdArgs a)
{
    const int s = fold_site(a.first_block, a.count);
    const int local = (int)blockIdx.x - a.first_block[s];
    const int c = a.c[s], n = a.n[s];
    const float eps = a.eps[s];
    const float* __restrict__ gamma = a.gamma[s];
    const float* __restrict__ var = a.var[s];
    if (local == 0) {
        const float* __restrict__ beta = a.beta[s];
        const float* __restrict__ mean = a.mean[s];
        float* __restrict__ t_out = a.t_out[s];
        for (int ch = threadIdx.x; ch < c; ch += FOLD_THREADS) {
            const float sc = gamma[ch] * fold_rstd(var[ch], eps);
            t_out[ch] = beta[ch] - mean[ch] * sc;
        }
    }
    const int base = local * FOLD_CHUNK;
    const int end = base + FOLD_CHUNK < n ? base + FOLD_CHUNK : n;
    fold_scale_chunk(a.w[s], a.w_out[s], gamma, var, eps, c, a.inner[s], base, end, a.vec[s]);
}

// dgamma_c = rstd_c * (S_c - mean_c * dt_c), S_c = sum over (outer, inner) of dw_out * w
__device__ __forceinline__ float fold_dgamma(float sum, float var, float eps, float mean, float dt)
{
    return fold_rstd(var, eps) * (sum - mean * dt);
}

__global__ __launch_bounds__(FOLD_THREADS) void bn_fold_bwd_kernel(const FoldBwdArgs a)
{
    __shared__ float part[FOLD_THREADS];
    const int s = fold_site(a.first_block, a.count);
    const int local = (int)blockIdx.x - a.first_block[s];
    const int c = a.c[s], inner = a.inner[s], n = a.n[s];
    const float eps = a.eps[s];
    const float* __restrict__ var = a.var[s];
    const float* __restrict__ dt = a.dt_out[s];
    if (local == 0 && a.dbeta[s]) {
        float* __restrict__ dbeta = a.dbeta[s];
        for (int ch = threadIdx.x; ch < c; ch += FOLD_THREADS) dbeta[ch] = dt ? dt[ch] : 0.0f;
    }
    if (local < a.ew_blocks[s]) {
        if (!a.dw[s]) return;                       // (a workgroup that exists for dbeta alone)
        const int base = local * FOLD_CHUNK;
        const int end = base + FOLD_CHUNK < n ? base + FOLD_CHUNK : n;
        fold_scale_chunk(a.dw_out[s], a.dw[s], a.gamma[s], var, eps, c, inner, base, end, a.vec[s]);
        return;
    }
    const int unit = local - a.ew_blocks[s];
    const float* __restrict__ w = a.w[s];
    const float* __restrict__ g = a.dw_out[s];
    const float* __restrict__ mean = a.mean[s];
    float* __restrict__ dgamma = a.dgamma[s];
    const int tile = a.tile[s];
    if (tile == 0) {
        // row sums: one wave per channel; lane l adds elements l, l + 64, ... of every outer slice in index order, then the
        // lanes fold by xor-shuffles
        const int ch = unit * FOLD_ROW_CH + ((int)threadIdx.x >> 6);
        if (ch >= c) return;
        const int outer = n / (c * inner);
        float acc = 0.0f;
        if (g)
            for (int o = 0; o < outer; ++o) {
                const int64_t row = ((int64_t)o * c + ch) * inner;
                for (int i = ws_lane(); i < inner; i += 64) acc = acc + g[row + i] * w[row + i];
            }
        acc = ws_wave_sum(acc);
        if (ws_lane() == 0) dgamma[ch] = fold_dgamma(acc, var[ch], eps, mean[ch], dt ? dt[ch] : 0.0f);
        return;
    }
    // column sums (inner == 1: the weight is [rows, c], the channel fastest): `tile` columns x 256 / tile row lanes; lane r adds
    // rows r, r + lanes, ... in order, then the lanes of a column are added in lane order
    const int lanes = FOLD_THREADS / tile;
    const int cl = (int)threadIdx.x % tile, rl = (int)threadIdx.x / tile;
    const int ch = unit * tile + cl;
    const int rows = n / c;
    float acc = 0.0f;
    if (g && ch < c) {
#pragma unroll 4
        for (int r = rl; r < rows; r += lanes) {
            const int64_t e = (int64_t)r * c + ch;
            acc = acc + g[e] * w[e];
        }
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    if (rl == 0 && ch < c) {
        float sum = part[cl];
        for (int l = 1; l < lanes; ++l) sum = sum + part[l * tile + cl];
        dgamma[ch] = fold_dgamma(sum, var[ch], eps, mean[ch], dt ? dt[ch] : 0.0f);
    }
}

int fold_check_site(int t, int64_t outer, int32_t c, int64_t inner, float eps)
{
    WS_REQUIRE(c >= 0, "site %d: bad channel count %d", t, c);
    if (c == 0) return WS_OK;
    WS_REQUIRE(outer >= 1 && inner >= 1, "site %d: bad shape [%lld, %d, %lld]", t, (long long)outer, c, (long long)inner);
    WS_REQUIRE(eps >= 0.0f, "site %d: negative eps", t);
    WS_REQUIRE(outer < (1ll << 31) && inner < (1ll << 31) && outer * c < (1ll << 31) && outer * c * inner < (1ll << 31) - FOLD_CHUNK,
               "site %d: weight too large [%lld, %d, %lld]", t, (long long)outer, c, (long long)inner);
    return WS_OK;
}

int fold_check_table(const void* h_w, const int64_t* h_outer, const int32_t* h_c, const int64_t* h_inner, const void* h_gamma,
                     const void* h_mean, const void* h_var, const float* h_eps, int32_t count)
{
    WS_REQUIRE(count >= 0, "bad site count %d", count);
    if (count == 0) return WS_OK;
    WS_REQUIRE(h_w && h_outer && h_c && h_inner && h_gamma && h_mean && h_var && h_eps, "NULL argument");
    for (int t = 0; t < count; ++t)
        if (int rc = fold_check_site(t, h_outer[t], h_c[t], h_inner[t], h_eps[t])) return rc;
    return WS_OK;
}

}  // namespace

extern "C" {

int ws_bn_fold_fwd(const float* const* h_w, const int64_t* h_outer, const int32_t* h_c, const int64_t* h_inner,
                   const float* const* h_gamma, const float* const* h_beta, const float* const* h_mean, const float* const* h_var,
                   const float* h_eps, float* const* h_w_out, float* const* h_t_out, int32_t count, void* stream)
{
    if (int rc = fold_check_table(h_w, h_outer, h_c, h_inner, h_gamma, h_mean, h_var, h_eps, count)) return rc;
    if (count == 0) return WS_OK;
    WS_REQUIRE(h_beta && h_w_out && h_t_out, "NULL argument");
    for (int t = 0; t < count; ++t)
        WS_REQUIRE(h_c[t] == 0 || (h_w[t] && h_gamma[t] && h_beta[t] && h_mean[t] && h_var[t] && h_w_out[t] && h_t_out[t]),
                   "NULL tensor of site %d", t);
    hipStream_t st = (hipStream_t)stream;
    int t = 0;
    while (t < count) {
        FoldFwdArgs a;
        a.count = 0;
        int blocks = 0;
        for (; t < count && a.count < FOLD_MAX; ++t) {
            if (h_c[t] == 0) continue;
            const FoldPlan p = fold_plan(h_outer[t], h_c[t], h_inner[t], h_w[t], h_w_out[t], false, true, false);
            const int j = a.count++;
            a.w[j] = h_w[t]; a.gamma[j] = h_gamma[t]; a.beta[j] = h_beta[t]; a.mean[j] = h_mean[t]; a.var[j] = h_var[t];
            a.w_out[j] = h_w_out[t]; a.t_out[j] = h_t_out[t];
            a.eps[j] = h_eps[t];
            a.c[j] = h_c[t]; a.inner[j] = (int)h_inner[t]; a.n[j] = (int)p.n;
            a.vec[j] = (unsigned char)p.vec;
            a.first_block[j] = blocks;
            blocks += p.ew_blocks;
        }
        if (a.count == 0) break;
        a.first_block[a.count] = blocks;
        bn_fold_fwd_kernel<<<blocks, FOLD_THREADS, 0, st>>>(a);
        WS_LAUNCH_CHECK();
    }
    return WS_OK;
}

int ws_bn_fold_bwd(const float* const* h_w, const int64_t* h_outer, const int32_t* h_c, const int64_t* h_inner,
                   const float* const* h_gamma, const float* const* h_mean, const float* const* h_var, const float* h_eps,
                   const float* const* h_dw_out, const float* const* h_dt_out, float* const* h_dw, float* const* h_dgamma,
                   float* const* h_dbeta, int32_t count, void* stream)
{
    if (int rc = fold_check_table(h_w, h_outer, h_c, h_inner, h_gamma, h_mean, h_var, h_eps, count)) return rc;
    if (count == 0) return WS_OK;
    WS_REQUIRE(h_dw_out && h_dt_out && h_dw && h_dgamma && h_dbeta, "NULL argument");
    for (int t = 0; t < count; ++t)
        WS_REQUIRE(h_c[t] == 0 || (h_w[t] && h_gamma[t] && h_mean[t] && h_var[t]), "NULL tensor of site %d", t);
    hipStream_t st = (hipStream_t)stream;
    int t = 0;
    while (t < count) {
        FoldBwdArgs a;
        a.count = 0;
        int blocks = 0;
        for (; t < count && a.count < FOLD_MAX; ++t) {
            if (h_c[t] == 0 || !(h_dw[t] || h_dgamma[t] || h_dbeta[t])) continue;
            FoldPlan p = fold_plan(h_outer[t], h_c[t], h_inner[t], h_dw_out[t], h_dw[t], true, h_dw[t] != nullptr, h_dgamma[t] != nullptr);
            if (p.ew_blocks + p.red_blocks == 0) p.ew_blocks = 1;           // dbeta alone
            const int j = a.count++;
            a.w[j] = h_w[t]; a.gamma[j] = h_gamma[t]; a.mean[j] = h_mean[t]; a.var[j] = h_var[t];
            a.dw_out[j] = h_dw_out[t]; a.dt_out[j] = h_dt_out[t];
            a.dw[j] = h_dw[t]; a.dgamma[j] = h_dgamma[t]; a.dbeta[j] = h_dbeta[t];
            a.eps[j] = h_eps[t];
            a.c[j] = h_c[t]; a.inner[j] = (int)h_inner[t]; a.n[j] = (int)p.n;
            a.ew_blocks[j] = p.ew_blocks;
            a.vec[j] = (unsigned char)p.vec; a.tile[j] = (unsigned char)p.tile;
            a.first_block[j] = blocks;
            blocks += p.ew_blocks + p.red_blocks;
        }
        if (a.count == 0) break;
        a.first_block[a.count] = blocks;
        bn_fold_bwd_kernel<<<blocks, FOLD_THREADS, 0, st>>>(a);
        WS_LAUNCH_CHECK();
    }
    return WS_OK;
}

int ws_bn_fold_variant(int32_t backward, int64_t outer, int32_t c, int64_t inner, const void* src, const void* dst, int32_t count,
                       char* text, int32_t cap)
{
    WS_REQUIRE(text && cap > 0, "bad argument");
    WS_REQUIRE(count >= 0, "bad site count %d", count);
    if (int rc = fold_check_site(0, outer, c, inner, 0.0f)) return rc;
    const int launches = (int)ws_ceil_div(count, FOLD_MAX);
    if (c == 0 || count == 0) {
        snprintf(text, (size_t)cap, "none (%s) launches=%d", c == 0 ? "c == 0" : "no sites", c == 0 ? 0 : launches);
        return WS_OK;
    }
    const FoldPlan p = fold_plan(outer, c, inner, src, dst, backward != 0, true, true);
    if (backward)
        snprintf(text, (size_t)cap, "bn_fold_bwd_kernel %s %s tile=%d ew_blocks=%d sum_blocks=%d launches=%d", p.vec ? "vector" : "scalar",
                 p.tile ? "column-sum" : "row-sum", p.tile ? p.tile : FOLD_ROW_CH, p.ew_blocks, p.red_blocks, launches);
    else
        snprintf(text, (size_t)cap, "bn_fold_fwd_kernel %s blocks=%d launches=%d", p.vec ? "vector" : "scalar", p.ew_blocks, launches);
    return WS_OK;
}

}  // extern "C"
