// weasal_amd/csrc/mprm_head.hip -- what follows the attention blocks in the weak-label step (KPFCNN_mprm, BASELINE config 1):
//
//   ws_segment_mean_fwd / _bwd   models/blocks.py:114-134 (global_average: split / mean / stack per sphere)
//   ws_max_heads_fwd / _bwd      models/architectures.py:700-702 (the nested torch.max over the four class-activation maps)
//   ws_bce_heads_fwd / _bwd      models/architectures.py:709-733, 778-783 (BCEWithLogitsLoss(weight = class_w) per path, summed)
//
// The four paths lie side by side in one [rows, heads * c] tensor.  All arithmetic is float32, there is no float atomic and
// every sum runs in an order fixed by the shapes alone: results are run-to-run bit-identical.  Sphere offsets travel in the
// kernel arguments (as in attention.hip); nothing is read back.
#include "ws_common.h"

namespace {

constexpr int MH_MAX_SPHERES = 64;     // WS_ATT_MAX_SPHERES
constexpr int MH_MAX_WIDTH = 1024;     // WS_SEGMENT_MAX_WIDTH
constexpr int MH_MAX_HEADS = 8;        // WS_HEADS_MAX
constexpr int SM_COLS = 64;            // columns of a segment_mean workgroup; its 4 waves take rows r, r + 4, ...
constexpr int BCE_THREADS = 1024;

struct SphereOffsets {
    int start[MH_MAX_SPHERES + 1];
    int count;
};

int sphere_offsets(const int64_t* lengths, int32_t nspheres, int64_t n, SphereOffsets& so)
{
    WS_REQUIRE(nspheres >= 0 && (nspheres == 0 || lengths), "bad sphere count %d or NULL lengths", nspheres);
    if (nspheres > MH_MAX_SPHERES)
        return ws_fail(WS_ERR_UNSUPPORTED, "%d spheres: at most %d travel in the kernel arguments", nspheres, MH_MAX_SPHERES);
    WS_REQUIRE(n >= 0 && n < (1ll << 31), "bad row count %lld", (long long)n);
    int64_t sum = 0;
    for (int s = 0; s < nspheres; ++s) {
        WS_REQUIRE(lengths[s] >= 0, "sphere %d: negative length %lld", s, (long long)lengths[s]);
        so.start[s] = (int)sum;
        sum += lengths[s];
        WS_REQUIRE(sum <= n, "the sphere lengths exceed the %lld rows", (long long)n);
    }
    WS_REQUIRE(sum == n, "the sphere lengths sum to %lld, not to the %lld rows", (long long)sum, (long long)n);
    so.start[nspheres] = (int)sum;
    so.count = nspheres;
    return WS_OK;
}

// ---- per-sphere mean ---------------------------------------------------------------------------------------------------
// grid (spheres, column chunks of 64), 256 threads: wave v sums the rows start + v, start + v + 4, ... of its column in row
// order, the four partial sums are added in wave order, then ONE division by the length (torch: sum, then / n; 0 / 0 = nan
// for an empty sphere).
__global__ __launch_bounds__(256) void segment_mean_fwd_kernel(const float* __restrict__ x, int64_t ldx, int w, const SphereOffsets so,
                                                               float* __restrict__ out)
{
    __shared__ float part[4][SM_COLS];
    const int s = blockIdx.x;
    const int col = blockIdx.y * SM_COLS + (threadIdx.x & 63);
    const int wave = threadIdx.x >> 6;
    const int beg = so.start[s], end = so.start[s + 1];
    float acc = 0.0f;
    if (col < w) {
        const float* xp = x + col;
        int r = beg + wave;
        for (; r + 12 < end; r += 16) {          // four independent loads in flight, added in row order
            const float a = xp[(int64_t)r * ldx], b = xp[(int64_t)(r + 4) * ldx], c = xp[(int64_t)(r + 8) * ldx],
                        d = xp[(int64_t)(r + 12) * ldx];
            acc = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(acc, a), b), c), d);
        }
        for (; r < end; r += 4) acc = __fadd_rn(acc, xp[(int64_t)r * ldx]);
    }
    part[wave][threadIdx.x & 63] = acc;
    __syncthreads();
    if (wave == 0 && col < w) {
        const int l = threadIdx.x;
        const float sum = __fadd_rn(__fadd_rn(__fadd_rn(part[0][l], part[1][l]), part[2][l]), part[3][l]);
        out[(int64_t)s * w + col] = __fdiv_rn(sum, (float)(end - beg));
    }
}

// one thread per element of dx [n, w]: the sphere of the row by binary search on the (scalar) offsets
__global__ __launch_bounds__(256) void segment_mean_bwd_kernel(const float* __restrict__ d_out, int64_t ldd, int w, int64_t total,
                                                               const SphereOffsets so, float* __restrict__ dx)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int row = (int)(e / w), col = (int)(e - (int64_t)row * w);
    int lo = 0, hi = so.count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (so.start[mid] <= row) lo = mid; else hi = mid;
    }
    dx[e] = __fdiv_rn(d_out[(int64_t)lo * ldd + col], (float)(so.start[lo + 1] - so.start[lo]));
}

// ---- maximum over heads ------------------------------------------------------------------------------------------------
// torch.max(a, b) of two tensors is torch.maximum: a nan on either side is the result.
__device__ __forceinline__ float max_nan(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }

__global__ __launch_bounds__(256) void max_heads_fwd_kernel(const float* __restrict__ x, int64_t ldx, int c, int heads, int64_t total,
                                                            float* __restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t row = e / c;
    const float* xp = x + row * ldx + (e - row * c);
    float m = xp[0];
    for (int k = 1; k < heads; ++k) m = max_nan(m, xp[(int64_t)k * c]);
    out[e] = m;
}

// autograd's rule for maximum(a, b) (derivatives.yaml): both sides start from (a == b ? g / 2 : g); a's is zeroed where
// a < b, b's where a > b.  Replayed from the outermost maximum inwards, as the nested expression's graph runs.
__global__ __launch_bounds__(256) void max_heads_bwd_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ d_out,
                                                            int64_t ldd, int c, int heads, int64_t total, float* __restrict__ dx)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t row = e / c;
    const int col = (int)(e - row * c);
    const float* xp = x + row * ldx + col;
    float h[MH_MAX_HEADS], m[MH_MAX_HEADS];
#pragma unroll
    for (int k = 0; k < MH_MAX_HEADS; ++k) {
        if (k < heads) {
            h[k] = xp[(int64_t)k * c];
            m[k] = k == 0 ? h[0] : max_nan(m[k - 1], h[k]);
        }
    }
    float* dp = dx + row * (int64_t)heads * c + col;
    float g = d_out[row * ldd + col];
#pragma unroll
    for (int k = MH_MAX_HEADS - 1; k >= 1; --k) {
        if (k < heads) {
            const float a = m[k - 1], b = h[k];
            const float both = a == b ? __fmul_rn(g, 0.5f) : g;
            dp[(int64_t)k * c] = a > b ? 0.0f : both;
            g = a < b ? 0.0f : both;
        }
    }
    dp[0] = g;
}

// ---- BCE with logits, `heads` column blocks against one target --------------------------------------------------------
__device__ __forceinline__ float bce_term(float x, float y)
{
    return __fadd_rn(__fadd_rn(fmaxf(x, 0.0f), -__fmul_rn(x, y)), log1pf(expf(-fabsf(x))));
}

// ONE workgroup of 1024 threads (the inputs are [regions or spheres, heads * classes]: some ten thousand elements).  Per head:
// thread t adds the elements t, t + 1024, ... in that order, the 64 lanes of a wave fold by xor-shuffles, the 16 wave sums
// are added in wave order; the per-head means are added in head order.  out[0 .. heads) = the means, out[heads] = their sum.
__global__ __launch_bounds__(BCE_THREADS) void bce_heads_fwd_kernel(const float* __restrict__ x, int64_t ldx, int r, int c, int heads,
                                                                    const float* __restrict__ target, const float* __restrict__ weight,
                                                                    float* __restrict__ out)
{
    __shared__ float wsum[BCE_THREADS / 64];
    const int per_head = r * c;
    float total = 0.0f;
    for (int k = 0; k < heads; ++k) {
        float acc = 0.0f;
        for (int e = threadIdx.x; e < per_head; e += BCE_THREADS) {
            const int row = e / c, col = e - row * c;
            float v = bce_term(x[(int64_t)row * ldx + k * c + col], target[e]);
            if (weight) v = __fmul_rn(v, weight[col]);
            acc = __fadd_rn(acc, v);
        }
        acc = ws_wave_sum(acc);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            float s = wsum[0];
            for (int i = 1; i < BCE_THREADS / 64; ++i) s = __fadd_rn(s, wsum[i]);
            const float mean = __fdiv_rn(s, (float)per_head);
            out[k] = mean;
            total = k == 0 ? mean : __fadd_rn(total, mean);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[heads] = total;
}

// dx[row, k c + col] = (g_heads[k] + g_sum) * weight[col] * (sigmoid(x) - y) / (r c); g_heads / g_sum: device floats, either NULL
__global__ __launch_bounds__(256) void bce_heads_bwd_kernel(const float* __restrict__ x, int64_t ldx, int c, int heads, int64_t total,
                                                            const float* __restrict__ target, const float* __restrict__ weight,
                                                            const float* __restrict__ g_heads, const float* __restrict__ g_sum,
                                                            float count, float* __restrict__ dx)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int hc = heads * c;
    const int64_t row = e / hc;
    const int j = (int)(e - row * hc), k = j / c, col = j - k * c;
    const float g = __fadd_rn(g_heads ? g_heads[k] : 0.0f, g_sum ? g_sum[0] : 0.0f);
    const float v = x[row * ldx + j];
    const float t = expf(-fabsf(v));
    const float sig = v >= 0.0f ? __fdiv_rn(1.0f, __fadd_rn(1.0f, t)) : __fdiv_rn(t, __fadd_rn(1.0f, t));
    float d = __fmul_rn(__fadd_rn(sig, -target[row * c + col]), g);
    if (weight) d = __fmul_rn(d, weight[col]);
    dx[e] = __fdiv_rn(d, count);
}

int elementwise_grid(int64_t total, int* blocks)
{
    WS_REQUIRE(total >= 0 && total < (1ll << 31) * 256, "too many elements (%lld)", (long long)total);
    *blocks = (int)ws_ceil_div(total, 256);
    return WS_OK;
}

}  // namespace

extern "C" {

int ws_segment_mean_fwd(const float* x, int64_t n, int32_t w, int64_t ldx, const int64_t* lengths, int32_t nspheres, float* out,
                        void* stream)
{
    if (w < 1 || w > MH_MAX_WIDTH) return ws_fail(WS_ERR_UNSUPPORTED, "segment_mean takes 1 to %d columns (got %d)", MH_MAX_WIDTH, w);
    WS_REQUIRE(ldx >= w, "row stride %lld below the width %d", (long long)ldx, w);
    SphereOffsets so;
    if (int rc = sphere_offsets(lengths, nspheres, n, so)) return rc;
    if (nspheres == 0) return WS_OK;
    WS_REQUIRE((x || n == 0) && out, "NULL argument");
    segment_mean_fwd_kernel<<<dim3(nspheres, (unsigned)ws_ceil_div(w, SM_COLS)), 256, 0, (hipStream_t)stream>>>(x, ldx, w, so, out);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_segment_mean_bwd(const float* d_out, int64_t ldd, int64_t n, int32_t w, const int64_t* lengths, int32_t nspheres, float* dx,
                        void* stream)
{
    if (w < 1 || w > MH_MAX_WIDTH) return ws_fail(WS_ERR_UNSUPPORTED, "segment_mean takes 1 to %d columns (got %d)", MH_MAX_WIDTH, w);
    WS_REQUIRE(ldd >= w, "row stride %lld below the width %d", (long long)ldd, w);
    SphereOffsets so;
    if (int rc = sphere_offsets(lengths, nspheres, n, so)) return rc;
    if (n == 0) return WS_OK;
    WS_REQUIRE(d_out && dx, "NULL argument");
    int blocks;
    if (int rc = elementwise_grid(n * w, &blocks)) return rc;
    segment_mean_bwd_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(d_out, ldd, w, n * w, so, dx);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_max_heads_fwd(const float* x, int64_t n, int32_t c, int32_t heads, int64_t ldx, float* out, void* stream)
{
    WS_REQUIRE(n >= 0 && c >= 1, "bad shape n %lld c %d", (long long)n, c);
    if (heads < 1 || heads > MH_MAX_HEADS) return ws_fail(WS_ERR_UNSUPPORTED, "1 to %d heads (got %d)", MH_MAX_HEADS, heads);
    WS_REQUIRE(ldx >= (int64_t)heads * c, "row stride %lld below heads * c = %lld", (long long)ldx, (long long)heads * c);
    if (n == 0) return WS_OK;
    WS_REQUIRE(x && out, "NULL argument");
    int blocks;
    if (int rc = elementwise_grid(n * c, &blocks)) return rc;
    max_heads_fwd_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(x, ldx, c, heads, n * c, out);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_max_heads_bwd(const float* x, int64_t n, int32_t c, int32_t heads, int64_t ldx, const float* d_out, int64_t ldd, float* dx,
                     void* stream)
{
    WS_REQUIRE(n >= 0 && c >= 1, "bad shape n %lld c %d", (long long)n, c);
    if (heads < 1 || heads > MH_MAX_HEADS) return ws_fail(WS_ERR_UNSUPPORTED, "1 to %d heads (got %d)", MH_MAX_HEADS, heads);
    WS_REQUIRE(ldx >= (int64_t)heads * c && ldd >= c, "row stride below the width");
    if (n == 0) return WS_OK;
    WS_REQUIRE(x && d_out && dx, "NULL argument");
    int blocks;
    if (int rc = elementwise_grid(n * c, &blocks)) return rc;
    max_heads_bwd_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(x, ldx, d_out, ldd, c, heads, n * c, dx);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_bce_heads_fwd(const float* x, int64_t r, int32_t c, int32_t heads, int64_t ldx, const float* target, const float* weight,
                     float* out, void* stream)
{
    WS_REQUIRE(r >= 1 && c >= 1, "bad shape r %lld c %d (an empty input has no mean)", (long long)r, c);
    if (heads < 1 || heads > MH_MAX_HEADS) return ws_fail(WS_ERR_UNSUPPORTED, "1 to %d heads (got %d)", MH_MAX_HEADS, heads);
    WS_REQUIRE(r * c < (1ll << 24), "%lld x %d elements per head: the count must be exact in float32", (long long)r, c);
    WS_REQUIRE(ldx >= (int64_t)heads * c, "row stride %lld below heads * c = %lld", (long long)ldx, (long long)heads * c);
    WS_REQUIRE(x && target && out, "NULL argument");
    bce_heads_fwd_kernel<<<1, BCE_THREADS, 0, (hipStream_t)stream>>>(x, ldx, (int)r, c, heads, target, weight, out);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_bce_heads_bwd(const float* x, int64_t r, int32_t c, int32_t heads, int64_t ldx, const float* target, const float* weight,
                     const float* g_heads, const float* g_sum, float* dx, void* stream)
{
    WS_REQUIRE(r >= 1 && c >= 1, "bad shape r %lld c %d (an empty input has no mean)", (long long)r, c);
    if (heads < 1 || heads > MH_MAX_HEADS) return ws_fail(WS_ERR_UNSUPPORTED, "1 to %d heads (got %d)", MH_MAX_HEADS, heads);
    WS_REQUIRE(r * c < (1ll << 24), "%lld x %d elements per head: the count must be exact in float32", (long long)r, c);
    WS_REQUIRE(ldx >= (int64_t)heads * c, "row stride %lld below heads * c = %lld", (long long)ldx, (long long)heads * c);
    WS_REQUIRE(x && target && dx && (g_heads || g_sum), "NULL argument");
    const int64_t total = r * heads * c;
    int blocks;
    if (int rc = elementwise_grid(total, &blocks)) return rc;
    bce_heads_bwd_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(x, ldx, c, heads, total, target, weight, g_heads, g_sum,
                                                                 (float)(r * c), dx);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

}  // extern "C"
