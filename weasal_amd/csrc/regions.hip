// weasal_amd/csrc/regions.hip -- the per-sphere regions of the weak-label sampler and the region means of the overlap-region loss.
//
//   ws_region_cut_count   datasets/DALES_WeakLabel.py:433-449   per (sphere, anchor of its tile): candidate? members inside?
//   ws_region_cut_scan    :449-451, :474-476                    slots and offsets of the kept regions, totals, per-sphere class rows
//   ws_region_cut_fill    :445-451                              the kept regions as CSR rows of the stacked batch
//   ws_region_mean_fwd    models/architectures.py:752-768       out[r] = mean of the rows of region r
//   ws_region_mean_bwd    (its backward)                        a gather through the transpose point -> regions
//
// Arithmetic (compiled with -ffp-contract=off): candidate iff d2 = (dx*dx + dy*dy) + dz*dz <= r*r in float64, d = anchor centre -
// sphere centre, every product and sum rounded.  Everything else of the cut is integers.  The means accumulate in float32 in an order
// fixed by the launch shape alone: no float atomics, the same bytes on every run.
//
// A wave owns 64 consecutive anchors of one sphere: every lane tests one centre, then the wave walks the candidates one after the
// other, its lanes laid over the anchor's members, each binary-searched in the sphere's ascending slice of input_inds.
#include "ws_scan.h"

namespace {

typedef unsigned long long u64;

constexpr int RG_BLOCK = 256;

struct CutArgs {
    const double* centres;          // [A, 3] of the tile
    const int64_t* a_ptr;           // [A + 1]
    const int64_t* a_idx;           // [a_nnz]
    const uint32_t* a_bits;         // [A] (fill)
    int64_t a_nnz, n_anchors;
    const int32_t* group;           // [n_group] spheres of the batch cut from this tile
    int n_group, n_spheres;
    const double* sph_centre;       // [B, 3]
    const int64_t* row_off;         // [B + 1]
    const int64_t* pair_off;        // [B + 1]
    const int64_t* input_inds;      // [n_rows]
    int64_t n_rows, pairs;
    double r2;
};

// first position of the ascending slice whose value is >= key
__device__ __forceinline__ int64_t lower_bound(const int64_t* __restrict__ v, int64_t n, int64_t key)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (v[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi)
{
    return v < lo ? lo : (v > hi ? hi : v);
}

template <bool FILL>
__global__ __launch_bounds__(RG_BLOCK) void cut_kernel(CutArgs c, int32_t* __restrict__ cnt, const int32_t* __restrict__ slot,
                                                       const int32_t* __restrict__ ptr32, int64_t n_regions, int64_t nnz, int n_class,
                                                       int64_t* __restrict__ out_ptr, int64_t* __restrict__ out_idx,
                                                       int32_t* __restrict__ out_reg, int32_t* __restrict__ out_sphere,
                                                       int64_t* __restrict__ out_anchor, float* __restrict__ out_lb,
                                                       float* __restrict__ out_inv_len)
{
    const int lane = ws_lane();
    const int64_t chunks = (c.n_anchors + 63) / 64;
    const int64_t n_waves = (int64_t)c.n_group * chunks;
    for (int64_t w = (int64_t)blockIdx.x * (RG_BLOCK / 64) + (threadIdx.x >> 6); w < n_waves; w += (int64_t)gridDim.x * (RG_BLOCK / 64)) {
        const int s = c.group[w / chunks];
        const int64_t a0 = (w % chunks) * 64;
        if (s < 0 || s >= c.n_spheres) continue;                                   // (all of these are the same in every lane)
        const int64_t r0 = c.row_off[s], r1 = c.row_off[s + 1], p0 = c.pair_off[s];
        if (r0 < 0 || r1 < r0 || r1 > c.n_rows || p0 < 0 || p0 + c.n_anchors > c.pairs) continue;
        const int64_t* __restrict__ slice = c.input_inds + r0;
        const int64_t n = r1 - r0;
        const int64_t a = a0 + lane;
        bool cand = false;
        if (a < c.n_anchors) {
            if (!FILL) {
                const double dx = c.centres[a * 3] - c.sph_centre[s * 3], dy = c.centres[a * 3 + 1] - c.sph_centre[s * 3 + 1],
                             dz = c.centres[a * 3 + 2] - c.sph_centre[s * 3 + 2];
                cand = (dx * dx + dy * dy) + dz * dz <= c.r2;
                if (!cand) cnt[p0 + a] = 0;
            } else {
                cand = cnt[p0 + a] > 0;
            }
        }
        u64 todo = __ballot(cand);
        while (todo) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int64_t aa = a0 + l;
            const int64_t mb = clamp64(c.a_ptr[aa], 0, c.a_nnz), me = clamp64(c.a_ptr[aa + 1], mb, c.a_nnz);
            if (!FILL) {
                int found = 0;
                bool nonzero = false;
                for (int64_t j = mb + lane; j < me; j += 64) {
                    const int64_t key = c.a_idx[j];
                    const int64_t pos = lower_bound(slice, n, key);
                    if (pos < n && slice[pos] == key) {
                        ++found;
                        nonzero |= pos != 0;
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) found += __shfl_xor(found, o, 64);
                const bool keep = __any(nonzero);                                   // `if idx.any()` (:449): some local row is not 0
                if (lane == 0) cnt[p0 + aa] = keep ? found : 0;
            } else {
                const int64_t r = slot[p0 + aa], base = ptr32[p0 + aa];
                const int64_t len = cnt[p0 + aa];
                if (r < 0 || r >= n_regions || base < 0 || base + len > nnz) continue;
                int64_t done = 0;
                for (int64_t j0 = mb; j0 < me; j0 += 64) {
                    const int64_t j = j0 + lane;
                    int64_t pos = 0;
                    bool hit = false;
                    if (j < me) {
                        const int64_t key = c.a_idx[j];
                        pos = lower_bound(slice, n, key);
                        hit = pos < n && slice[pos] == key;
                    }
                    const u64 hits = __ballot(hit);
                    const int64_t at = done + __popcll(hits & ((1ull << lane) - 1ull));
                    if (hit && at < len) {
                        out_idx[base + at] = r0 + pos;
                        out_reg[base + at] = (int32_t)r;
                    }
                    done += __popcll(hits);
                }
                if (lane == 0) {
                    out_ptr[r] = base;
                    out_sphere[r] = s;
                    out_anchor[r] = aa;
                    out_inv_len[r] = 1.0f / (float)len;
                }
                if (lane < n_class) out_lb[r * n_class + lane] = (float)((c.a_bits[aa] >> lane) & 1u);
            }
        }
    }
}

__global__ __launch_bounds__(RG_BLOCK) void flags_kernel(const int32_t* __restrict__ cnt, int64_t n, int32_t* __restrict__ flags)
{
    for (int64_t i = (int64_t)blockIdx.x * RG_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * RG_BLOCK) flags[i] = cnt[i] > 0;
}

__global__ void totals_kernel(const int32_t* __restrict__ slot_end, const int32_t* __restrict__ ptr_end, int64_t* __restrict__ words)
{
    if (threadIdx.x == 0) {
        words[WS_REGION_TOTAL_ROWS] = *slot_end;
        words[WS_REGION_TOTAL_NNZ] = *ptr_end;
    }
}

// one workgroup per sphere: the OR of 1 << label over its rows, unpacked into cloud_lb[s, :]
__global__ __launch_bounds__(RG_BLOCK) void cloud_lb_kernel(const int64_t* __restrict__ labels, const int64_t* __restrict__ row_off,
                                                            int64_t n_rows, int n_class, float* __restrict__ cloud_lb,
                                                            int64_t* __restrict__ words)
{
    __shared__ unsigned seen;
    __shared__ unsigned bad;
    if (threadIdx.x == 0) { seen = 0u; bad = 0u; }
    __syncthreads();
    const int s = blockIdx.x;
    const int64_t r0 = clamp64(row_off[s], 0, n_rows), r1 = clamp64(row_off[s + 1], r0, n_rows);
    unsigned mine = 0u, wrong = 0u;
    for (int64_t i = r0 + threadIdx.x; i < r1; i += RG_BLOCK) {
        const int64_t lb = labels[i];
        if (lb >= 0 && lb < n_class) mine |= 1u << (int)lb;
        else ++wrong;
    }
    if (mine) atomicOr(&seen, mine);
    if (wrong) atomicAdd(&bad, wrong);
    __syncthreads();
    if ((int)threadIdx.x < n_class) cloud_lb[(int64_t)s * n_class + threadIdx.x] = (float)((seen >> threadIdx.x) & 1u);
    if (threadIdx.x == 0 && bad) atomicAdd((u64*)words + WS_REGION_BAD_LABEL, (u64)bad);
}

// ---- region means ----------------------------------------------------------------------------------------------------
// One workgroup per region.  wp = the power of two >= w: thread t serves column t % wp of the rows sub, sub + 256 / wp, ...
// (sub = t / wp), so that the lanes of a wave read the w floats of a row side by side; the 256 / wp partial sums of a column
// meet in LDS and are added in ascending sub.
__global__ __launch_bounds__(RG_BLOCK) void region_mean_fwd_kernel(const float* __restrict__ x, int64_t n, int w, int wp_log2,
                                                                   const int64_t* __restrict__ ptr, const int64_t* __restrict__ idx,
                                                                   int64_t nnz, const float* __restrict__ inv_len, int64_t n_regions,
                                                                   float* __restrict__ out)
{
    __shared__ float part[RG_BLOCK];
    const int wp = 1 << wp_log2, rpp = RG_BLOCK >> wp_log2;
    const int col = threadIdx.x & (wp - 1), sub = threadIdx.x >> wp_log2;
    for (int64_t r = blockIdx.x; r < n_regions; r += gridDim.x) {
        const int64_t b = clamp64(ptr[r], 0, nnz), e = clamp64(ptr[r + 1], b, nnz);
        float acc = 0.0f;
        if (col < w) {
            int64_t i = b + sub;
            for (; i + 3 * (int64_t)rpp < e; i += 4 * (int64_t)rpp) {              // four rows in flight
                const int64_t q0 = idx[i], q1 = idx[i + rpp], q2 = idx[i + 2 * rpp], q3 = idx[i + 3 * rpp];
                const float v0 = (q0 >= 0 && q0 < n) ? x[q0 * w + col] : 0.0f;
                const float v1 = (q1 >= 0 && q1 < n) ? x[q1 * w + col] : 0.0f;
                const float v2 = (q2 >= 0 && q2 < n) ? x[q2 * w + col] : 0.0f;
                const float v3 = (q3 >= 0 && q3 < n) ? x[q3 * w + col] : 0.0f;
                acc += v0;
                acc += v1;
                acc += v2;
                acc += v3;
            }
            for (; i < e; i += rpp) {
                const int64_t q = idx[i];
                if (q >= 0 && q < n) acc += x[q * w + col];
            }
        }
        part[threadIdx.x] = acc;
        __syncthreads();
        if (sub == 0 && col < w) {
            float sum = part[col];
            for (int k = 1; k < rpp; ++k) sum += part[k * wp + col];
            out[r * w + col] = sum * inv_len[r];
        }
        __syncthreads();
    }
}

// 256 / wp rows per workgroup, a thread per (row, column): every element of dx is stored, a row in no region as 0
__global__ __launch_bounds__(RG_BLOCK) void region_mean_bwd_kernel(const float* __restrict__ g, int64_t n_regions, int w, int wp_log2,
                                                                   const int64_t* __restrict__ t_ptr, const int32_t* __restrict__ t_reg,
                                                                   int64_t nnz, const float* __restrict__ inv_len, int64_t n,
                                                                   float* __restrict__ dx)
{
    const int wp = 1 << wp_log2, rpp = RG_BLOCK >> wp_log2;
    const int col = threadIdx.x & (wp - 1), sub = threadIdx.x >> wp_log2;
    if (col >= w) return;
    for (int64_t row = (int64_t)blockIdx.x * rpp + sub; row < n; row += (int64_t)gridDim.x * rpp) {
        const int64_t b = clamp64(t_ptr[row], 0, nnz), e = clamp64(t_ptr[row + 1], b, nnz);
        float acc = 0.0f;
        for (int64_t i = b; i < e; ++i) {
            const int64_t r = t_reg[i];
            if (r >= 0 && r < n_regions) acc += g[r * w + col] * inv_len[r];
        }
        dx[row * w + col] = acc;
    }
}

int cut_args(CutArgs& c, const char* who, const double* centres, const int64_t* a_ptr, const int64_t* a_idx, int64_t a_nnz,
             int64_t n_anchors, const int32_t* group, int32_t n_group, int32_t n_spheres, const double* sph_centre,
             const int64_t* row_off, const int64_t* pair_off, const int64_t* input_inds, int64_t n_rows, int64_t pairs)
{
    WS_REQUIRE(n_anchors >= 1 && a_nnz >= 0 && n_group >= 1 && n_spheres >= 1 && n_rows >= 0 && pairs >= n_anchors,
               "%s: bad sizes anchors=%lld nnz=%lld group=%d spheres=%d rows=%lld pairs=%lld", who, (long long)n_anchors, (long long)a_nnz,
               n_group, n_spheres, (long long)n_rows, (long long)pairs);
    if (n_spheres > WS_REGION_MAX_SPHERES || n_group > n_spheres)
        return ws_fail(WS_ERR_UNSUPPORTED, "%s: %d spheres, %d in the group (at most %d)", who, n_spheres, n_group, WS_REGION_MAX_SPHERES);
    if (pairs >= (1ll << 31)) return ws_fail(WS_ERR_UNSUPPORTED, "%s: %lld (sphere, anchor) pairs (below 2^31)", who, (long long)pairs);
    WS_REQUIRE(a_ptr && (a_nnz == 0 || a_idx) && group && row_off && pair_off && (n_rows == 0 || input_inds), "%s: NULL argument", who);
    c = CutArgs{centres, a_ptr, a_idx, nullptr, a_nnz, n_anchors, group, n_group, n_spheres, sph_centre, row_off, pair_off, input_inds,
                n_rows, pairs, 0.0};
    return WS_OK;
}

int cut_grid(const CutArgs& c)
{
    return ws_grid((int64_t)c.n_group * ((c.n_anchors + 63) / 64), RG_BLOCK / 64, 1 << 14);
}

int mean_shape(const char* who, int32_t w, int& wp_log2)
{
    if (w < 1 || w > WS_REGION_MAX_WIDTH) return ws_fail(WS_ERR_UNSUPPORTED, "%s: width %d (1 to %d columns)", who, w, WS_REGION_MAX_WIDTH);
    wp_log2 = 0;
    while ((1 << wp_log2) < w) ++wp_log2;
    return WS_OK;
}

}  // namespace

extern "C" {

int64_t ws_region_scratch_bytes(int64_t pairs)
{
    const int64_t p = pairs < 0 ? 0 : pairs;
    return (int64_t)sizeof(int32_t) * (ws_scan_scratch_items(p) + p + 1);
}

int ws_region_cut_count(const double* centres, const int64_t* anchor_ptr, const int64_t* anchor_idx, int64_t anchor_nnz,
                        int64_t n_anchors, const int32_t* group, int32_t n_group, int32_t n_spheres, const double* sphere_centres,
                        const int64_t* row_off, const int64_t* pair_off, const int64_t* input_inds, int64_t n_rows, int64_t pairs,
                        double radius, int32_t* cnt, void* stream)
{
    CutArgs c;
    int rc = cut_args(c, "ws_region_cut_count", centres, anchor_ptr, anchor_idx, anchor_nnz, n_anchors, group, n_group, n_spheres,
                      sphere_centres, row_off, pair_off, input_inds, n_rows, pairs);
    if (rc) return rc;
    WS_REQUIRE(centres && sphere_centres && cnt && radius >= 0.0, "ws_region_cut_count: NULL argument or radius=%g", radius);
    c.r2 = radius * radius;
    cut_kernel<false><<<cut_grid(c), RG_BLOCK, 0, (hipStream_t)stream>>>(c, cnt, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, nullptr,
                                                                        nullptr, nullptr, nullptr, nullptr);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_region_cut_scan(int32_t* cnt, int64_t pairs, int32_t* slot, int32_t* ptr32, const int64_t* labels, const int64_t* row_off,
                       int64_t n_rows, int32_t n_spheres, int32_t n_class, float* cloud_lb, int64_t* words, void* scratch, void* stream)
{
    WS_REQUIRE(pairs >= 0 && n_rows >= 0 && n_spheres >= 1, "ws_region_cut_scan: bad sizes pairs=%lld rows=%lld spheres=%d",
               (long long)pairs, (long long)n_rows, n_spheres);
    if (n_class < 1 || n_class > 32) return ws_fail(WS_ERR_UNSUPPORTED, "ws_region_cut_scan: n_class=%d (1 to 32)", n_class);
    if (n_spheres > WS_REGION_MAX_SPHERES || pairs >= (1ll << 31))
        return ws_fail(WS_ERR_UNSUPPORTED, "ws_region_cut_scan: spheres=%d (at most %d), pairs=%lld (below 2^31)", n_spheres,
                       WS_REGION_MAX_SPHERES, (long long)pairs);
    WS_REQUIRE(row_off && cloud_lb && words && (n_rows == 0 || labels) && (pairs == 0 || (cnt && slot && ptr32 && scratch)),
               "ws_region_cut_scan: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    WS_HIP(hipMemsetAsync(words, 0, sizeof(int64_t) * WS_REGION_WORDS, st));
    cloud_lb_kernel<<<n_spheres, RG_BLOCK, 0, st>>>(labels, row_off, n_rows, n_class, cloud_lb, words);
    WS_LAUNCH_CHECK();
    if (pairs == 0) return WS_OK;
    int32_t* flags = (int32_t*)scratch;
    int32_t* scan_scratch = flags + pairs + 1;
    flags_kernel<<<ws_grid(pairs, RG_BLOCK * 4, 1024), RG_BLOCK, 0, st>>>(cnt, pairs, flags);
    WS_LAUNCH_CHECK();
    int rc = ws_exclusive_scan_i32(flags, slot, pairs, scan_scratch, st);
    if (rc) return rc;
    rc = ws_exclusive_scan_i32(cnt, ptr32, pairs, scan_scratch, st);
    if (rc) return rc;
    totals_kernel<<<1, 64, 0, st>>>(slot + pairs, ptr32 + pairs, words);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_region_cut_fill(const int64_t* anchor_ptr, const int64_t* anchor_idx, int64_t anchor_nnz, const uint32_t* anchor_bits,
                       int64_t n_anchors, const int32_t* group, int32_t n_group, int32_t n_spheres, const int64_t* row_off,
                       const int64_t* pair_off, const int64_t* input_inds, int64_t n_rows, int64_t pairs, const int32_t* cnt,
                       const int32_t* slot, const int32_t* ptr32, int64_t n_regions, int64_t nnz, int32_t n_class, int64_t* out_ptr,
                       int64_t* out_idx, int32_t* out_reg, int32_t* out_sphere, int64_t* out_anchor, float* out_lb, float* out_inv_len,
                       void* stream)
{
    CutArgs c;
    int rc = cut_args(c, "ws_region_cut_fill", nullptr, anchor_ptr, anchor_idx, anchor_nnz, n_anchors, group, n_group, n_spheres, nullptr,
                      row_off, pair_off, input_inds, n_rows, pairs);
    if (rc) return rc;
    WS_REQUIRE(n_regions >= 0 && nnz >= 0, "ws_region_cut_fill: bad sizes regions=%lld nnz=%lld", (long long)n_regions, (long long)nnz);
    if (n_class < 1 || n_class > 32) return ws_fail(WS_ERR_UNSUPPORTED, "ws_region_cut_fill: n_class=%d (1 to 32)", n_class);
    if (n_regions == 0) return WS_OK;
    WS_REQUIRE(anchor_bits && cnt && slot && ptr32 && out_ptr && out_idx && out_reg && out_sphere && out_anchor && out_lb && out_inv_len,
               "ws_region_cut_fill: NULL argument");
    c.a_bits = anchor_bits;
    cut_kernel<true><<<cut_grid(c), RG_BLOCK, 0, (hipStream_t)stream>>>(c, const_cast<int32_t*>(cnt), slot, ptr32, n_regions, nnz, n_class,
                                                                       out_ptr, out_idx, out_reg, out_sphere, out_anchor, out_lb,
                                                                       out_inv_len);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_region_mean_fwd(const float* x, int64_t n, int32_t w, const int64_t* region_ptr, const int64_t* region_idx, int64_t nnz,
                       const float* inv_len, int64_t n_regions, float* out, void* stream)
{
    WS_REQUIRE(n >= 0 && nnz >= 0 && n_regions >= 0, "ws_region_mean_fwd: bad sizes n=%lld nnz=%lld regions=%lld", (long long)n,
               (long long)nnz, (long long)n_regions);
    int wp_log2;
    int rc = mean_shape("ws_region_mean_fwd", w, wp_log2);
    if (rc) return rc;
    if (n_regions == 0) return WS_OK;
    WS_REQUIRE(region_ptr && inv_len && out && (nnz == 0 || (region_idx && x)), "ws_region_mean_fwd: NULL argument");
    region_mean_fwd_kernel<<<ws_grid(n_regions, 1, 1 << 14), RG_BLOCK, 0, (hipStream_t)stream>>>(x, n, w, wp_log2, region_ptr, region_idx, nnz,
                                                                                               inv_len, n_regions, out);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_region_mean_bwd(const float* grad_out, int64_t n_regions, int32_t w, const int64_t* t_ptr, const int32_t* t_reg, int64_t nnz,
                       const float* inv_len, int64_t n, float* grad_x, void* stream)
{
    WS_REQUIRE(n >= 0 && nnz >= 0 && n_regions >= 0, "ws_region_mean_bwd: bad sizes n=%lld nnz=%lld regions=%lld", (long long)n,
               (long long)nnz, (long long)n_regions);
    int wp_log2;
    int rc = mean_shape("ws_region_mean_bwd", w, wp_log2);
    if (rc) return rc;
    if (n == 0) return WS_OK;
    WS_REQUIRE(t_ptr && grad_x && (nnz == 0 || (t_reg && grad_out && inv_len)), "ws_region_mean_bwd: NULL argument");
    region_mean_bwd_kernel<<<ws_grid(n, RG_BLOCK >> wp_log2, 1 << 14), RG_BLOCK, 0, (hipStream_t)stream>>>(grad_out, n_regions, w, wp_log2,
                                                                                                        t_ptr, t_reg, nnz, inv_len, n,
                                                                                                        grad_x);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

}  // extern "C"
