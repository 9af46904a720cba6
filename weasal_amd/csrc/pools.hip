// weasal_amd/csrc/pools.hip -- max_pool / closest_pool (models/blocks.py:80-111) forward and
// backward.  Rows are contiguous (4*c bytes): lanes run along the channel axis so that every
// access is a coalesced row segment; the backward forms gather through the transposed table
// (csr.hip) instead of the reference's scatter_add.
#include "ws_common.h"
#include <algorithm>
#include "ws_dispatch.h"

namespace {

__device__ __forceinline__ int64_t ws_ceil_div_dev(int64_t a, int64_t b) { return (a + b - 1) / b; }
bool al16p(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
__device__ __forceinline__ int4 load_arg4(const int32_t* p) { return *reinterpret_cast<const int4*>(p); }
__device__ __forceinline__ int4 load_arg4(const uint8_t* p)
{
    const unsigned w = *reinterpret_cast<const unsigned*>(p);
    return make_int4((int)(w & 0xffu), (int)((w >> 8) & 0xffu), (int)((w >> 16) & 0xffu), (int)(w >> 24));
}

// VEC path (c % 4 == 0, 16-byte aligned rows): G = c/4 lanes (capped at 64) cover one row with
// float4 pieces, 64/G query rows per wave, the neighbour loop unrolled by 4 so that four row
// gathers are in flight per lane; shadow columns read nothing (zero row, blocks.py:104).
// AT = the element type of the arg-max record: int32 (the C ABI), or uint8 inside the block calls when h <= 255 -- the
// backward reads one arg piece per (incoming pair, row piece), 2.7 GB at level 0 with 4-byte elements
// Work assignment of the vectorised pools.  ilv = 0: every workgroup takes one contiguous chunk of the (spatially ordered)
// group list (ws_block_range).  ilv > 0 (workgroups per XCD; grid = 8 x ilv): the workgroups of an XCD walk ITS eighth of
// the list together, group g = base + (local workgroup) * 4 + wave + t * (ilv * 4): at any moment the XCD works on ~ilv * 4
// * S neighbouring queries, whose gathered rows fit its 4 MB L2 (with contiguous chunks the resident workgroups sit at
// chunk starts spread over the whole cloud: every row came from the fabric again, FETCH_SIZE ~ the logical bytes).
__device__ __forceinline__ void pool_groups(int64_t ngroups, int ilv, int wave, int64_t& g0, int64_t& gstep, int64_t& gend)
{
    if (ilv > 0 && (gridDim.x & 7) == 0) {
        const int x = blockIdx.x & 7, lb = blockIdx.x >> 3, nbx = gridDim.x >> 3;
        const int64_t per8 = (ngroups + 7) / 8;
        const int64_t b8 = (int64_t)x * per8;
        gend = b8 + per8 < ngroups ? b8 + per8 : ngroups;
        g0 = b8 + (int64_t)lb * 4 + wave;
        gstep = (int64_t)nbx * 4;
    } else {
        int64_t ibeg, iend;
        ws_block_range(ngroups, ibeg, iend);
        g0 = ibeg + wave; gstep = 4; gend = iend;
    }
}

template <int G, typename T, typename AT = int32_t, int U = 4>
__global__ __launch_bounds__(256) void max_pool_fwd_vec_kernel(const T* __restrict__ x, int64_t ns, int c,
                                                                const int64_t* __restrict__ inds, int64_t nq, int h,
                                                                T* __restrict__ out, AT* __restrict__ arg,
                                                                const int32_t* __restrict__ order = nullptr, int ilv = 0, int split = 1)
{
    // split > 1 (wide rows of few queries: the deep levels): a group = (query, one 4 G-channel chunk) instead of a query with
    // its chunks one after the other -- 275 queries x 1 024 channels are 1 100 independent waves instead of 275 four times as long
    // order (optional): a spatially coherent permutation of the queries (the cell order of their level's search).  The
    // pooled points come out of the grid subsampling in hash-table order: walked by index, consecutive queries gather
    // rows from all over the cloud and every 512-byte row is fetched ~3.6 times from HBM (PMC, round 2); in cell order
    // the waves of a workgroup share their neighbourhoods in L2.
    constexpr int S = 64 / G;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int j = lane % G, slot = lane / G;
    int64_t g0, gstep, gend;
    pool_groups(ws_ceil_div_dev(nq, S) * split, ilv, wave, g0, gstep, gend);
    for (int64_t grp = g0; grp < gend; grp += gstep) {
        const int64_t qi = (grp / split) * S + slot;
        const bool qok = qi < nq;
        const int64_t q = (qok && order) ? (int64_t)order[qi] : qi;
        const int cbeg = split > 1 ? (int)(grp % split) * (4 * G) : 0;
        const int cend = split > 1 ? min(cbeg + 4 * G, c) : c;
        for (int c0 = cbeg; c0 < cend; c0 += 4 * G) {
            const int ch = c0 + 4 * j;
            const bool ok = qok && ch < c;
            float4 best = make_float4(-3.4e38f, -3.4e38f, -3.4e38f, -3.4e38f);
            int bi[4] = {0, 0, 0, 0};
            for (int h0 = 0; h0 < h; h0 += U) {            // U neighbour rows in flight per lane
                float4 v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                    const int col = h0 + u;
                    int64_t s = (ok && col < h) ? inds[q * h + col] : -1;
                    if (s >= 0 && s < ns) v[u] = ld4(x + s * c + ch);
                    else if (col >= h) v[u] = make_float4(-3.4e38f, -3.4e38f, -3.4e38f, -3.4e38f);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {               // first maximum wins
                    if (v[u].x > best.x) { best.x = v[u].x; bi[0] = h0 + u; }
                    if (v[u].y > best.y) { best.y = v[u].y; bi[1] = h0 + u; }
                    if (v[u].z > best.z) { best.z = v[u].z; bi[2] = h0 + u; }
                    if (v[u].w > best.w) { best.w = v[u].w; bi[3] = h0 + u; }
                }
            }
            if (ok) {
                st4(out + q * c + ch, best);
                if (arg) {
                    if constexpr (sizeof(AT) == 4)
                        *reinterpret_cast<int4*>(arg + q * c + ch) = make_int4(bi[0], bi[1], bi[2], bi[3]);
                    else
                        *reinterpret_cast<unsigned*>(arg + q * c + ch) =
                            (unsigned)bi[0] | ((unsigned)bi[1] << 8) | ((unsigned)bi[2] << 16) | ((unsigned)bi[3] << 24);
                }
            }
        }
    }
}

// generic path: one wave per query row; lanes stride over channels
template <typename T>
__global__ __launch_bounds__(256) void max_pool_fwd_kernel(const T* __restrict__ x, int64_t ns, int c,
                                                            const int64_t* __restrict__ inds, int64_t nq, int h,
                                                            T* __restrict__ out, int32_t* __restrict__ arg)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (int64_t q = (int64_t)blockIdx.x * 4 + wave; q < nq; q += (int64_t)gridDim.x * 4) {
        for (int c0 = 0; c0 < c; c0 += 64) {
            const int ch = c0 + lane;
            float best = -3.4e38f;
            int bi = 0;
            for (int j = 0; j < h; ++j) {
                const int64_t s = inds[q * h + j];           // wave-uniform
                float v = 0.0f;                               // shadow row = zeros (blocks.py:104)
                if (s >= 0 && s < ns && ch < c) v = ld1(x + s * c + ch);
                if (v > best) { best = v; bi = j; }           // first maximum wins
            }
            if (ch < c) {
                st1(out + q * c + ch, best);
                if (arg) arg[q * c + ch] = bi;
            }
        }
    }
}

// backward, VEC path: G lanes x float4 per support row, 64/G supports per wave
template <int G, typename T, typename AT = int32_t>
__global__ __launch_bounds__(256) void max_pool_bwd_vec_kernel(const T* __restrict__ dy, const AT* __restrict__ arg,
                                                                int h, int c, const int32_t* __restrict__ t_offsets,
                                                                const int32_t* __restrict__ t_pairs, int64_t ns,
                                                                T* __restrict__ dx, const int32_t* __restrict__ order = nullptr,
                                                                int ilv = 0, const T* __restrict__ add = nullptr, int split = 1)
{
    // split: as in the forward -- a group = (support, one channel chunk)
    // add (same shape as dx, or NULL): a second gradient of the same rows, summed into the store -- dx = pool gradient + add
    constexpr int S = 64 / G;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int j = lane % G, slot = lane / G;
    int64_t g0, gstep, gend;
    pool_groups(ws_ceil_div_dev(ns, S) * split, ilv, wave, g0, gstep, gend);
    for (int64_t grp = g0; grp < gend; grp += gstep) {
        const int64_t si = (grp / split) * S + slot;
        const bool sok = si < ns;
        const int64_t s = (sok && order) ? (int64_t)order[si] : si;       // supports in their level's cell order (see the forward)
        const int beg = sok ? t_offsets[s] : 0, end = sok ? t_offsets[s + 1] : 0;
        const int cbeg = split > 1 ? (int)(grp % split) * (4 * G) : 0;
        const int cend = split > 1 ? min(cbeg + 4 * G, c) : c;
        for (int c0 = cbeg; c0 < cend; c0 += 4 * G) {
            const int ch = c0 + 4 * j;
            if (!(sok && ch < c)) continue;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            // a channel of a pooled row takes its maximum from ONE of the h neighbours: of the incoming pairs of s only
            // ~ 1 / h carry a gradient for a given channel.  So the arg-max pieces of four pairs are fetched together and
            // a piece of dy only where one of its four channels matches (same sums, in the same order; half the bytes)
            int p = beg;
            for (; p + 3 < end; p += 4) {
                int q4[4], col4[4];
                int4 a4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int pair = t_pairs[p + u];
                    q4[u] = pair / h;
                    col4[u] = pair - q4[u] * h;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) a4[u] = load_arg4(arg + (int64_t)q4[u] * c + ch);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int4 a = a4[u];
                    const int col = col4[u];
                    if (a.x == col || a.y == col || a.z == col || a.w == col) {
                        const float4 g = ld4(dy + (int64_t)q4[u] * c + ch);
                        if (a.x == col) acc.x += g.x;
                        if (a.y == col) acc.y += g.y;
                        if (a.z == col) acc.z += g.z;
                        if (a.w == col) acc.w += g.w;
                    }
                }
            }
            for (; p < end; ++p) {
                const int pair = t_pairs[p];
                const int q = pair / h, col = pair - q * h;
                const int4 a = load_arg4(arg + (int64_t)q * c + ch);
                if (a.x == col || a.y == col || a.z == col || a.w == col) {
                    const float4 g = ld4(dy + (int64_t)q * c + ch);
                    if (a.x == col) acc.x += g.x;
                    if (a.y == col) acc.y += g.y;
                    if (a.z == col) acc.z += g.z;
                    if (a.w == col) acc.w += g.w;
                }
            }
            if (add) { const float4 o = ld4(add + s * c + ch); acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w; }
            st4(dx + s * c + ch, acc);
        }
    }
}

// one wave per support row
template <typename T>
__global__ __launch_bounds__(256) void max_pool_bwd_kernel(const T* __restrict__ dy, const int32_t* __restrict__ arg,
                                                            int h, int c, const int32_t* __restrict__ t_offsets,
                                                            const int32_t* __restrict__ t_pairs, int64_t ns,
                                                            T* __restrict__ dx)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (int64_t s = (int64_t)blockIdx.x * 4 + wave; s < ns; s += (int64_t)gridDim.x * 4) {
        const int beg = t_offsets[s], end = t_offsets[s + 1];
        for (int c0 = 0; c0 < c; c0 += 64) {
            const int ch = c0 + lane;
            float acc = 0.0f;
            if (ch < c) {
                for (int p = beg; p < end; ++p) {
                    const int pair = t_pairs[p];
                    const int q = pair / h, col = pair - q * h;
                    if (arg[(int64_t)q * c + ch] == col) acc += ld1(dy + (int64_t)q * c + ch);
                }
                st1(dx + s * c + ch, acc);
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void closest_pool_fwd_kernel(const T* __restrict__ x, int64_t ns, int c,
                                                                const int64_t* __restrict__ inds, int64_t nq, int h,
                                                                T* __restrict__ out)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (int64_t q = (int64_t)blockIdx.x * 4 + wave; q < nq; q += (int64_t)gridDim.x * 4) {
        const int64_t s = inds[q * h];
        const bool real = s >= 0 && s < ns;
        for (int ch = lane; ch < c; ch += 64) st1(out + q * c + ch, real ? ld1(x + s * c + ch) : 0.0f);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void closest_pool_bwd_kernel(const T* __restrict__ dy, int h, int c,
                                                                const int32_t* __restrict__ t_offsets,
                                                                const int32_t* __restrict__ t_pairs, int64_t ns,
                                                                T* __restrict__ dx)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (int64_t s = (int64_t)blockIdx.x * 4 + wave; s < ns; s += (int64_t)gridDim.x * 4) {
        const int beg = t_offsets[s], end = t_offsets[s + 1];
        for (int c0 = 0; c0 < c; c0 += 64) {
            const int ch = c0 + lane;
            float acc = 0.0f;
            if (ch < c) {
                for (int p = beg; p < end; ++p) {
                    const int pair = t_pairs[p];
                    const int q = pair / h;
                    if (pair - q * h == 0) acc += ld1(dy + (int64_t)q * c + ch);
                }
                st1(dx + s * c + ch, acc);
            }
        }
    }
}


// float rows of c = 4 G channels, G | 64: G lanes x float4 per incoming row, S = 64 / G rows of a support in flight side by side
// (and two trips unrolled), the S partial sums added in a fixed order at the end.  The scalar form above walks a support's
// fine points one dependent 4-byte-per-lane load at a time: 95 us for the 400 000 -> 71 000 level of the DALES step.
template <int G>
__global__ __launch_bounds__(256) void closest_pool_bwd_vec_kernel(const float* __restrict__ dy, int h, int c,
                                                                    const int32_t* __restrict__ t_offsets,
                                                                    const int32_t* __restrict__ t_pairs, int64_t ns,
                                                                    float* __restrict__ dx)
{
    constexpr int S = 64 / G;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int j = lane % G, slot = lane / G;
    for (int64_t s = (int64_t)blockIdx.x * 4 + wave; s < ns; s += (int64_t)gridDim.x * 4) {
        const int beg = t_offsets[s], end = t_offsets[s + 1];
        for (int c0 = 0; c0 < c; c0 += 4 * G) {              // (G < 64: c = 4 G, one trip; G = 64: 256 channels per trip)
            const int ch = c0 + 4 * j;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            int p = beg + slot;
            for (; p + S < end; p += 2 * S) {
                const int pa = t_pairs[p], pb = t_pairs[p + S];
                const int qa = pa / h, qb = pb / h;
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b4 = a;
                if (pa - qa * h == 0) a = *reinterpret_cast<const float4*>(dy + (int64_t)qa * c + ch);
                if (pb - qb * h == 0) b4 = *reinterpret_cast<const float4*>(dy + (int64_t)qb * c + ch);
                acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
                acc.x += b4.x; acc.y += b4.y; acc.z += b4.z; acc.w += b4.w;
            }
            if (p < end) {
                const int pa = t_pairs[p];
                const int qa = pa / h;
                if (pa - qa * h == 0) {
                    const float4 a = *reinterpret_cast<const float4*>(dy + (int64_t)qa * c + ch);
                    acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
                }
            }
#pragma unroll
            for (int o = G; o < 64; o <<= 1) {
                acc.x += __shfl_xor(acc.x, o, 64); acc.y += __shfl_xor(acc.y, o, 64);
                acc.z += __shfl_xor(acc.z, o, 64); acc.w += __shfl_xor(acc.w, o, 64);
            }
            if (slot == 0) *reinterpret_cast<float4*>(dx + s * c + ch) = acc;
        }
    }
}

// workgroups per XCD of the interleaved assignment (with a spatial order; without one: contiguous chunks).  Level-0 max-pool
// of the DALES step (71 000 x 59 rows of 512 bytes): forward 245 -> 195 us in the step, 136 -> 97 us alone
constexpr int POOL_INTERLEAVE = 256;
constexpr int POOL_SPLIT_ROWS = 8192;   // max-pools over fewer rows than this give every 256-channel chunk of a row a wave of its own
extern "C" int ws_closest_bwd_vec = 1;      // nearest-upsampling backward: 1 = float4 lanes, several incoming rows side by side (A/B: WEASAL_CLOSEST_BWD_VEC)

// ---- plans: what an entry launches, from its arguments alone (pointers only for their alignment).  The launchers below and the
//      reporter (ws_pool_variant) call the same plan function; every selection rule is here.
enum { PK_MAX_FWD_VEC, PK_MAX_FWD, PK_MAX_BWD_VEC, PK_MAX_BWD, PK_CLOSEST_FWD, PK_CLOSEST_BWD, PK_CLOSEST_BWD_VEC };
struct PoolPlan {
    int kernel;         // PK_*: the kernel family
    bool bf16;          // row type T: bf16_t instead of float
    int g;              // G: lanes per row (the vector forms)
    int u;              // U: neighbour rows in flight per lane (PK_MAX_FWD_VEC)
    int arg_bytes;      // AT of the arg-max record: 4 = int32_t (the C ABI), 1 = uint8_t (the block calls)
    int split;          // channel chunks of a row that are groups of their own (1: a row is one group)
    int ilv;            // workgroups per XCD of the interleaved assignment; 0: contiguous chunks
    int grid;           // workgroups of 256 threads
};
const char* row_name(const PoolPlan& p) { return p.bf16 ? "bf16" : "f32"; }

int pool_grid(int64_t groups, int ilv)
{
    if (ilv <= 0) return ws_grid(groups, 4);
    const int64_t need = (groups + 31) / 32;              // never more workgroups per XCD than groups / 4 / 8
    return 8 * (int)std::max<int64_t>(1, std::min<int64_t>(ilv, need));
}

// every max-pool entry.  fwd: rows = nq, a / b = x / out, arg may be NULL (which counts as aligned); backward: rows = ns,
// a / b = dy / dx.  arg_bytes = 1 (f32 rows in float4 pieces: the caller's precondition) has the vector forms only.
PoolPlan max_pool_plan(bool fwd, bool bf16, int64_t rows, int c, const void* a, const void* b, const void* arg, int arg_bytes, bool ordered)
{
    PoolPlan p{fwd ? PK_MAX_FWD : PK_MAX_BWD, bf16, 0, 0, arg_bytes, 1, 0, ws_grid(rows, 4)};      // one wave per row; takes no order
    const bool rows_al = bf16 ? ws_row_aligned<bf16_t>(a) && ws_row_aligned<bf16_t>(b) : ws_row_aligned<float>(a) && ws_row_aligned<float>(b);
    if (arg_bytes != 1 && !(c % 4 == 0 && rows_al && al16p(arg))) return p;
    p.kernel = fwd ? PK_MAX_FWD_VEC : PK_MAX_BWD_VEC;
    p.g = (fwd && c <= 16) ? 4 : (c <= 32 ? 8 : (c <= 64 ? 16 : (c <= 128 ? 32 : 64)));           // (the backward has no G = 4)
    // 128 channels: 8 neighbour rows in flight per lane (level 0 of the DALES step: 184 -> 172 us alone, against 4)
    p.u = (fwd && arg_bytes == 1 && p.g == 32) ? 8 : 4;
    p.split = (rows < POOL_SPLIT_ROWS && c > 256) ? (int)ws_ceil_div(c, 256) : 1;                 // (c > 256: G = 64)
    p.ilv = ordered ? POOL_INTERLEAVE : 0;               // (only with a spatial order is a neighbouring group a neighbouring place)
    p.grid = pool_grid(ws_ceil_div(rows, 64 / p.g) * p.split, p.ilv);
    return p;
}

PoolPlan closest_fwd_plan(bool bf16, int64_t nq) { return PoolPlan{PK_CLOSEST_FWD, bf16, 0, 0, 0, 1, 0, ws_grid(nq, 4)}; }

// vector form: f32 rows of c = 4 G channels, G | 64, or whole waves (G = 64) over rows of c % 256 == 0
PoolPlan closest_bwd_plan(bool bf16, int64_t ns, int c, const void* dy, const void* dx)
{
    PoolPlan p{PK_CLOSEST_BWD, bf16, 0, 0, 0, 1, 0, ws_grid(ns, 4)};
    if (!bf16 && ws_closest_bwd_vec && al16p(dy) && al16p(dx) && (c == 32 || c == 64 || c == 128 || c % 256 == 0)) {
        p.kernel = PK_CLOSEST_BWD_VEC;
        p.g = c % 256 == 0 ? 64 : c / 4;
    }
    return p;
}

// the name of a plan: what tests/test_pool_branches_*.py count and compare
void plan_text(const PoolPlan& p, char* out, size_t n)
{
    const char* op = (p.kernel == PK_MAX_FWD_VEC || p.kernel == PK_MAX_FWD) ? "max_fwd" : "max_bwd";
    switch (p.kernel) {
    case PK_MAX_FWD_VEC: case PK_MAX_BWD_VEC:
        snprintf(out, n, "%s vec G=%d U=%d AT=%s %s split=%d %s", op, p.g, p.u, p.arg_bytes == 1 ? "u8" : "i32", row_name(p), p.split,
                 p.ilv ? "interleaved" : "contiguous");
        break;
    case PK_MAX_FWD: case PK_MAX_BWD: snprintf(out, n, "%s generic %s", op, row_name(p)); break;
    case PK_CLOSEST_FWD: snprintf(out, n, "closest_fwd scalar %s", row_name(p)); break;
    case PK_CLOSEST_BWD: snprintf(out, n, "closest_bwd scalar %s", row_name(p)); break;
    default: snprintf(out, n, "closest_bwd vec G=%d", p.g);
    }
}

// ---- launchers: one dispatch on the plan per kernel family.  `hit` stays false where the plan names what is not instantiated
int launched(bool hit, const PoolPlan& p)
{
    if (!hit) return ws_no_instantiation("pool kernel family %d <G=%d, U=%d> bf16=%d arg_bytes=%d", p.kernel, p.g, p.u, p.bf16, p.arg_bytes);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

// the forwards: max_pool_fwd_vec_kernel (the byte record: f32 rows only; U = 8: its G = 32 form only), or a wave per row
// (max_pool_fwd_kernel, closest_pool_fwd_kernel)
int launch_fwd(const PoolPlan& p, void* stream, const void* x, int64_t ns, int32_t c, const int64_t* inds, int64_t nq, int32_t h, void* out,
               void* arg, const int32_t* order)
{
    hipStream_t st = (hipStream_t)stream;
    bool hit = false;
    if (p.kernel == PK_MAX_FWD_VEC)
        dispatch([&](auto bf, auto g, auto u, auto u8) {
            using T = Row<bf.value>;
            using AT = std::conditional_t<u8.value != 0, uint8_t, int32_t>;
            if constexpr (!(bf.value && u8.value) && (u.value == 8) == (u8.value && g.value == 32)) {
                max_pool_fwd_vec_kernel<g.value, T, AT, u.value><<<p.grid, 256, 0, st>>>((const T*)x, ns, c, inds, nq, h, (T*)out, (AT*)arg, order,
                                                                                         p.ilv, p.split);
                hit = true;
            }
        }, Flag{p.bf16}, Pick<4, 8, 16, 32, 64>{p.g}, Pick<4, 8>{p.u}, Flag{p.arg_bytes == 1});
    else
        hit = dispatch([&](auto bf) {
            using T = Row<bf.value>;
            if (p.kernel == PK_MAX_FWD) max_pool_fwd_kernel<T><<<p.grid, 256, 0, st>>>((const T*)x, ns, c, inds, nq, h, (T*)out, (int32_t*)arg);
            else closest_pool_fwd_kernel<T><<<p.grid, 256, 0, st>>>((const T*)x, ns, c, inds, nq, h, (T*)out);
        }, Flag{p.bf16});
    return launched(hit, p);
}

// the backwards: max_pool_bwd_vec_kernel (no G = 4; the byte record: f32 rows only; add: the byte-record entry's),
// closest_pool_bwd_vec_kernel (f32 rows), or a wave per row (max_pool_bwd_kernel, closest_pool_bwd_kernel)
int launch_bwd(const PoolPlan& p, void* stream, const void* dy, const void* arg, int32_t h, int32_t c, const int32_t* t_offsets,
               const int32_t* t_pairs, int64_t ns, void* dx, const int32_t* order, const float* add = nullptr)
{
    hipStream_t st = (hipStream_t)stream;
    bool hit = false;
    if (p.kernel == PK_MAX_BWD_VEC)
        dispatch([&](auto bf, auto g, auto u8) {
            using T = Row<bf.value>;
            using AT = std::conditional_t<u8.value != 0, uint8_t, int32_t>;
            if constexpr (!(bf.value && u8.value)) {
                max_pool_bwd_vec_kernel<g.value, T, AT><<<p.grid, 256, 0, st>>>((const T*)dy, (const AT*)arg, h, c, t_offsets, t_pairs, ns, (T*)dx,
                                                                                order, p.ilv, (const T*)add, p.split);
                hit = true;
            }
        }, Flag{p.bf16}, Pick<8, 16, 32, 64>{p.g}, Flag{p.arg_bytes == 1});
    else if (p.kernel == PK_CLOSEST_BWD_VEC)
        hit = dispatch([&](auto g) {
            closest_pool_bwd_vec_kernel<g.value><<<p.grid, 256, 0, st>>>((const float*)dy, h, c, t_offsets, t_pairs, ns, (float*)dx);
        }, Pick<8, 16, 32, 64>{p.g});
    else
        hit = dispatch([&](auto bf) {
            using T = Row<bf.value>;
            if (p.kernel == PK_MAX_BWD) max_pool_bwd_kernel<T><<<p.grid, 256, 0, st>>>((const T*)dy, (const int32_t*)arg, h, c, t_offsets, t_pairs, ns, (T*)dx);
            else closest_pool_bwd_kernel<T><<<p.grid, 256, 0, st>>>((const T*)dy, h, c, t_offsets, t_pairs, ns, (T*)dx);
        }, Flag{p.bf16});
    return launched(hit, p);
}

// ---- the public entries: validate, plan, launch.  closest: the closest pools, which have neither arg nor order
int pool_fwd_impl(bool closest, bool bf16, const void* x, int64_t ns, int32_t c, const int64_t* inds, int64_t nq, int32_t h, void* out,
                  int32_t* arg, const int32_t* order, void* stream)
{
    WS_REQUIRE(ns >= 0 && nq >= 0 && c >= 1 && h >= 1, "bad sizes");
    if (nq == 0) return WS_OK;
    WS_REQUIRE(inds && out && (ns == 0 || x), "NULL argument");
    const PoolPlan p = closest ? closest_fwd_plan(bf16, nq) : max_pool_plan(true, bf16, nq, c, x, out, arg, 4, order != nullptr);
    return launch_fwd(p, stream, x, ns, c, inds, nq, h, out, arg, order);
}

int pool_bwd_impl(bool closest, bool bf16, const void* dy, const int32_t* arg, int64_t nq, int32_t h, int32_t c, const int32_t* t_offsets,
                  const int32_t* t_pairs, int64_t ns, void* dx, const int32_t* order, void* stream)
{
    WS_REQUIRE(ns >= 0 && nq >= 0 && c >= 1 && h >= 1, "bad sizes");
    if (ns == 0) return WS_OK;
    WS_REQUIRE(t_offsets && dx && (nq == 0 || (dy && (closest || arg) && t_pairs)), "NULL argument");
    const PoolPlan p = closest ? closest_bwd_plan(bf16, ns, c, dy, dx) : max_pool_plan(false, bf16, ns, c, dy, dx, arg, 4, order != nullptr);
    return launch_bwd(p, stream, dy, arg, h, c, t_offsets, t_pairs, ns, dx, order);
}

}  // namespace

extern "C" {

int ws_max_pool_fwd(const float* x, int64_t ns, int32_t c, const int64_t* inds, int64_t nq, int32_t h,
                    float* out, int32_t* arg, void* stream)
{
    return pool_fwd_impl(false, false, x, ns, c, inds, nq, h, out, arg, nullptr, stream);
}

int ws_max_pool_bwd(const float* dy, const int32_t* arg, int64_t nq, int32_t h, int32_t c,
                    const int32_t* t_offsets, const int32_t* t_pairs, int64_t ns, float* dx, void* stream)
{
    return pool_bwd_impl(false, false, dy, arg, nq, h, c, t_offsets, t_pairs, ns, dx, nullptr, stream);
}

int ws_max_pool_fwd_ordered(const float* x, int64_t ns, int32_t c, const int64_t* inds, int64_t nq, int32_t h, float* out, int32_t* arg,
                            const int32_t* order_q, void* stream)
{
    return pool_fwd_impl(false, false, x, ns, c, inds, nq, h, out, arg, order_q, stream);
}

int ws_max_pool_bwd_ordered(const float* dy, const int32_t* arg, int64_t nq, int32_t h, int32_t c, const int32_t* t_offsets,
                            const int32_t* t_pairs, int64_t ns, float* dx, const int32_t* order_s, void* stream)
{
    return pool_bwd_impl(false, false, dy, arg, nq, h, c, t_offsets, t_pairs, ns, dx, order_s, stream);
}

int ws_max_pool_fwd_ordered_bf16(const uint16_t* x, int64_t ns, int32_t c, const int64_t* inds, int64_t nq, int32_t h, uint16_t* out,
                                 int32_t* arg, const int32_t* order_q, void* stream)
{
    return pool_fwd_impl(false, true, x, ns, c, inds, nq, h, out, arg, order_q, stream);
}

int ws_max_pool_bwd_ordered_bf16(const uint16_t* dy, const int32_t* arg, int64_t nq, int32_t h, int32_t c, const int32_t* t_offsets,
                                 const int32_t* t_pairs, int64_t ns, uint16_t* dx, const int32_t* order_s, void* stream)
{
    return pool_bwd_impl(false, true, dy, arg, nq, h, c, t_offsets, t_pairs, ns, dx, order_s, stream);
}

int ws_closest_pool_fwd(const float* x, int64_t ns, int32_t c, const int64_t* inds, int64_t nq, int32_t h,
                        float* out, void* stream)
{
    return pool_fwd_impl(true, false, x, ns, c, inds, nq, h, out, nullptr, nullptr, stream);
}

int ws_closest_pool_bwd(const float* dy, int64_t nq, int32_t h, int32_t c, const int32_t* t_offsets,
                        const int32_t* t_pairs, int64_t ns, float* dx, void* stream)
{
    return pool_bwd_impl(true, false, dy, nullptr, nq, h, c, t_offsets, t_pairs, ns, dx, nullptr, stream);
}

// bf16 feature rows (BASELINE config 5): same kernels, 8-byte row pieces
int ws_max_pool_fwd_bf16(const uint16_t* x, int64_t ns, int32_t c, const int64_t* inds, int64_t nq, int32_t h,
                         uint16_t* out, int32_t* arg, void* stream)
{
    return pool_fwd_impl(false, true, x, ns, c, inds, nq, h, out, arg, nullptr, stream);
}

int ws_max_pool_bwd_bf16(const uint16_t* dy, const int32_t* arg, int64_t nq, int32_t h, int32_t c,
                         const int32_t* t_offsets, const int32_t* t_pairs, int64_t ns, uint16_t* dx, void* stream)
{
    return pool_bwd_impl(false, true, dy, arg, nq, h, c, t_offsets, t_pairs, ns, dx, nullptr, stream);
}

int ws_closest_pool_fwd_bf16(const uint16_t* x, int64_t ns, int32_t c, const int64_t* inds, int64_t nq, int32_t h,
                             uint16_t* out, void* stream)
{
    return pool_fwd_impl(true, true, x, ns, c, inds, nq, h, out, nullptr, nullptr, stream);
}

int ws_closest_pool_bwd_bf16(const uint16_t* dy, int64_t nq, int32_t h, int32_t c, const int32_t* t_offsets,
                             const int32_t* t_pairs, int64_t ns, uint16_t* dx, void* stream)
{
    return pool_bwd_impl(true, true, dy, nullptr, nq, h, c, t_offsets, t_pairs, ns, dx, nullptr, stream);
}

// private to the library (declared in ws_common.h, not part of include/weasal_hip.h): the block calls keep their arg-max
// record in bytes.  Preconditions (checked by the caller): h <= 255, c % 4 == 0, 16-byte aligned rows, 4-byte aligned arg.
int ws_priv_max_pool_fwd_u8(const float* x, int64_t ns, int32_t c, const int64_t* inds, int64_t nq, int32_t h, float* out,
                            uint8_t* arg, const int32_t* order_q, void* stream)
{
    if (nq == 0) return WS_OK;
    return launch_fwd(max_pool_plan(true, false, nq, c, x, out, arg, 1, order_q != nullptr), stream, x, ns, c, inds, nq, h, out, arg, order_q);
}

int ws_priv_max_pool_bwd_u8(const float* dy, const uint8_t* arg, int64_t nq, int32_t h, int32_t c, const int32_t* t_offsets,
                            const int32_t* t_pairs, int64_t ns, float* dx, const int32_t* order_s, const float* add, void* stream)
{
    (void)nq;
    if (ns == 0) return WS_OK;
    return launch_bwd(max_pool_plan(false, false, ns, c, dy, dx, arg, 1, order_s != nullptr), stream, dy, arg, h, c, t_offsets, t_pairs, ns,
                          dx, order_s, add);
}

// What the entries of this file launch for these arguments, as the name tests/test_pool_branches_*.py count ("max_fwd vec G=32
// U=4 AT=i32 f32 split=1 interleaved", "max_bwd generic bf16", "closest_bwd vec G=16", ...): the plan function of the entry
// named by op (WS_POOL_*, weasal_hip.h), nothing read or launched.  rows = nq (forwards) or ns (backwards); rows_a / rows_b: the two
// row operands (x and out, or dy and dx) and arg: tested for alignment only.  grid (may be NULL): the workgroups of the launch.
int ws_pool_variant(int32_t op, int64_t rows, int32_t c, const void* rows_a, const void* rows_b, const void* arg, int32_t rows_bf16,
                    int32_t arg_bytes, int32_t ordered, char* out, int32_t cap, int32_t* grid)
{
    WS_REQUIRE(out && cap > 0 && rows >= 0 && c >= 1 && (arg_bytes == 4 || arg_bytes == 1), "bad argument");
    const bool bf = rows_bf16 != 0, max_op = op == WS_POOL_MAX_FWD || op == WS_POOL_MAX_BWD;
    WS_REQUIRE(arg_bytes == 4 || (max_op && !bf && c % 4 == 0 && al16p(rows_a) && al16p(rows_b) && (reinterpret_cast<uintptr_t>(arg) & 3u) == 0),
               "the byte arg-max record: max-pools of f32 rows, c %% 4 == 0, 16-byte aligned rows, 4-byte aligned arg");
    PoolPlan p;
    switch (op) {
    case WS_POOL_MAX_FWD: case WS_POOL_MAX_BWD: p = max_pool_plan(op == WS_POOL_MAX_FWD, bf, rows, c, rows_a, rows_b, arg, arg_bytes, ordered != 0); break;
    case WS_POOL_CLOSEST_FWD: p = closest_fwd_plan(bf, rows); break;
    case WS_POOL_CLOSEST_BWD: p = closest_bwd_plan(bf, rows, c, rows_a, rows_b); break;
    default: return ws_fail(WS_ERR_INVALID, "unknown pool operation %d", op);
    }
    plan_text(p, out, (size_t)cap);
    if (grid) *grid = p.grid;
    return WS_OK;
}

}  // extern "C"
