// weasal_amd/csrc/neighbors_kernels.h -- the device side of the radius search (K1): the kernels that build the cell grid and
// the query kernels that walk it.  Included by neighbors.hip alone (one translation unit, compiled with -ffp-contract=off:
// the distance recipe must round like the reference's, no FMA); the workspace, the fill plan and the entries are there.
// The walk itself -- cell block, runs, candidate batches, key layout, compaction -- is in ws_grid.h, shared with the
// grid-walk KPConv backward.
#pragma once
#include "ws_scan.h"
#include "ws_grid.h"

namespace {

__global__ __launch_bounds__(1024) void nb_bbox_kernel(const float* __restrict__ pts, CloudGrid* __restrict__ grids,
                                                        float* __restrict__ bbox /*[nb][6]*/)
{
    __shared__ float red[6][16];
    const CloudGrid g = grids[blockIdx.x];
    float mn[3] = {3.4e38f, 3.4e38f, 3.4e38f}, mx[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
    for (int i = threadIdx.x; i < g.s_len; i += blockDim.x) {
        const float* p = pts + 3 * (int64_t)(g.s_base + i);
#pragma unroll
        for (int d = 0; d < 3; ++d) { mn[d] = fminf(mn[d], p[d]); mx[d] = fmaxf(mx[d], p[d]); }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn[d] = fminf(mn[d], __shfl_xor(mn[d], o, 64));
            mx[d] = fmaxf(mx[d], __shfl_xor(mx[d], o, 64));
        }
        if (lane == 0) { red[d][wave] = mn[d]; red[3 + d][wave] = mx[d]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int d = threadIdx.x;
        float v = red[d][0];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) v = d < 3 ? fminf(v, red[d][w]) : fmaxf(v, red[d][w]);
        bbox[blockIdx.x * 6 + d] = v;
    }
}

// The per-element table travels as a kernel argument (copied at launch): no host staging buffer
// whose lifetime would force a stream synchronisation.
constexpr int GRID_TABLE_MAX = 48;
struct GridTable { CloudGrid g[GRID_TABLE_MAX]; };
__global__ void nb_upload_kernel(GridTable t, int nb, CloudGrid* __restrict__ dst)
{
    const int b = threadIdx.x;
    if (b < nb) dst[b] = t.g[b];
}

// grid reuse: only the query ranges of the per-element table change
struct QueryTable { int q_base[GRID_TABLE_MAX]; int q_len[GRID_TABLE_MAX]; };
__global__ void nb_update_queries_kernel(QueryTable t, int nb, CloudGrid* __restrict__ grids)
{
    const int b = threadIdx.x;
    if (b < nb) { grids[b].q_base = t.q_base[b]; grids[b].q_len = t.q_len[b]; }
}

__global__ void nb_grid_setup_kernel(CloudGrid* __restrict__ grids, const float* __restrict__ bbox, int nb, float radius)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    CloudGrid g = grids[b];
    if (g.s_len <= 0) {
        g.lo[0] = g.lo[1] = g.lo[2] = 0.f; g.inv_cell = 1.f; g.nx = g.ny = g.nz = 1;
        grids[b] = g;
        return;
    }
    const float* bb = bbox + 6 * b;
    // cell > radius by a margin that dominates the rounding of (v - lo) * inv_cell (dims <= 512)
    float cell = (radius > 0.f ? radius : 1.f) * 1.001f;
    int nx, ny, nz;
    for (;;) {
        const float inv = 1.0f / cell;
        nx = (int)floorf((bb[3] - bb[0]) * inv) + 1;
        ny = (int)floorf((bb[4] - bb[1]) * inv) + 1;
        nz = (int)floorf((bb[5] - bb[2]) * inv) + 1;
        if (nx <= 512 && ny <= 512 && nz <= 512 && (int64_t)nx * ny * nz <= (int64_t)g.cell_cap) break;
        cell *= 1.26f;
    }
    g.lo[0] = bb[0]; g.lo[1] = bb[1]; g.lo[2] = bb[2];
    g.inv_cell = 1.0f / cell;
    g.nx = nx; g.ny = ny; g.nz = nz;
    grids[b] = g;
}

// one thread per support: cell id + histogram
__global__ __launch_bounds__(256) void nb_bin_count_kernel(const float* __restrict__ pts, const CloudGrid* __restrict__ grids,
                                                            int nb, int64_t ns, int32_t* __restrict__ cell_of,
                                                            int32_t* __restrict__ cell_count)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < ns; i += (int64_t)gridDim.x * 256) {
        int b = 0;
        while (b + 1 < nb && i >= grids[b].s_base + grids[b].s_len) ++b;
        const CloudGrid& g = grids[b];
        const float* p = pts + 3 * i;
        int cx = min(max(cell_coord(p[0], g.lo[0], g.inv_cell), 0), g.nx - 1);
        int cy = min(max(cell_coord(p[1], g.lo[1], g.inv_cell), 0), g.ny - 1);
        int cz = min(max(cell_coord(p[2], g.lo[2], g.inv_cell), 0), g.nz - 1);
        const int c = g.cell_base + (cz * g.ny + cy) * g.nx + cx;
        cell_of[i] = c;
        atomicAdd(&cell_count[c], 1);
    }
}

__global__ __launch_bounds__(256) void nb_bin_fill_kernel(const float* __restrict__ pts, int64_t ns,
                                                           const int32_t* __restrict__ cell_of,
                                                           int32_t* __restrict__ cursor, float4* __restrict__ sorted)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < ns; i += (int64_t)gridDim.x * 256) {
        const int pos = atomicAdd(&cursor[cell_of[i]], 1);
        sorted[pos] = make_float4(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], __int_as_float((int)i));
    }
}

// Enumerate the candidates of query (qx,qy,qz): calls f(float4 cand) for all lanes in lock-step;
// every lane of the wave takes part, `cand.w` carries the global support index; inactive lanes
// get active=false.
template <typename F>
__device__ __forceinline__ void for_each_candidate(const CloudGrid& g, float qx, float qy, float qz,
                                                   const int32_t* __restrict__ cell_start,
                                                   const float4* __restrict__ sorted, int lane, F&& f)
{
    const int cx = cell_coord(qx, g.lo[0], g.inv_cell);
    const int cy = cell_coord(qy, g.lo[1], g.inv_cell);
    const int cz = cell_coord(qz, g.lo[2], g.inv_cell);
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.nx - 1);
    if (x0 > x1) return;
    for (int z = max(cz - 1, 0); z <= min(cz + 1, g.nz - 1); ++z) {
        for (int y = max(cy - 1, 0); y <= min(cy + 1, g.ny - 1); ++y) {
            const int row = g.cell_base + (z * g.ny + y) * g.nx;
            const int beg = cell_start[row + x0], end = cell_start[row + x1 + 1];
            for (int p0 = beg; p0 < end; p0 += 64) {
                const int p = p0 + lane;
                const bool active = p < end;
                float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
                if (active) c = sorted[p];
                f(c, active);
            }
        }
    }
}

// The running maximum of the row lengths lives in ONE word: 16 384 waves each ending in an atomicMax on it serialise at
// ~7.5 ns per atomic (measured: 0.9 ms per DALES pyramid, most of it exposed in the mid-size launches).  The maximum saturates
// after a few hundred rows, so a wave first reads the word (a stale value is only ever too small) and skips the atomic
// unless it would raise it.
__device__ __forceinline__ void nb_publish_max(int32_t* __restrict__ max_count, int local_max, int lane)
{
    if (lane == 0 && local_max > 0 &&
        local_max > __hip_atomic_load(max_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(max_count, local_max);
}

__device__ __forceinline__ int find_cloud_q(const CloudGrid* __restrict__ grids, int nb, int64_t q)
{
    int b = 0;
    while (b + 1 < nb && q >= grids[b].q_base + grids[b].q_len) ++b;
    return b;
}

__global__ __launch_bounds__(256) void nb_count_kernel(const float* __restrict__ queries, int64_t nq,
                                                        const CloudGrid* __restrict__ grids, int nb,
                                                        const int32_t* __restrict__ cell_start,
                                                        const float4* __restrict__ sorted, float r2,
                                                        const int32_t* __restrict__ qorder,
                                                        int32_t* __restrict__ counts, int32_t* __restrict__ max_count)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    int local_max = 0;
    int64_t ibeg, iend;
    ws_block_range(nq, ibeg, iend);
    for (int64_t it = ibeg + wave; it < iend; it += 4) {
        const int64_t q = qorder ? (int64_t)qorder[it] : it;
        const int b = find_cloud_q(grids, nb, q);
        const CloudGrid g = grids[b];
        const float qx = queries[3 * q], qy = queries[3 * q + 1], qz = queries[3 * q + 2];
        int cnt = 0;
        if (g.s_len > 0) {
            for_each_candidate(g, qx, qy, qz, cell_start, sorted, lane, [&](const float4& c, bool active) {
                const bool hit = active && ref_d2(qx, qy, qz, c) < r2;
                cnt += __builtin_popcountll(__ballot(hit));
            });
        }
        if (lane == 0) counts[q] = cnt;
        local_max = max(local_max, cnt);
    }
    nb_publish_max(max_count, local_max, lane);
}

// Count-only pass of the neighbourhood-limit calibration (datasets/DALES_PseudoLabel.py:1238-1240): the walk of nb_count_kernel,
// but what leaves the wave is one increment of bin [count] instead of a row length.  The bins of a workgroup's range live in
// LDS (hist_n ints, dynamic): one LDS add per query, by lane 0.  Only when the range is done do the non-zero bins go to `hist`,
// as 64-bit adds -- once per workgroup, not per query (see nb_publish_max for the price of per-wave atomics on one word).
// A count of hist_n or more is dropped: np.bincount(c, minlength=hist_n)[:hist_n] (:1239).  Integer adds only: the result
// does not depend on the arrival order.
__global__ __launch_bounds__(256) void nb_hist_kernel(const float* __restrict__ queries, int64_t nq,
                                                       const CloudGrid* __restrict__ grids, int nb,
                                                       const int32_t* __restrict__ cell_start,
                                                       const float4* __restrict__ sorted, float r2,
                                                       const int32_t* __restrict__ qorder,
                                                       unsigned long long* __restrict__ hist, int hist_n)
{
    extern __shared__ int nb_hist_bins[];      // [hist_n]; a workgroup's range is < 2^31 queries
    for (int i = threadIdx.x; i < hist_n; i += 256) nb_hist_bins[i] = 0;
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    int64_t ibeg, iend;
    ws_block_range(nq, ibeg, iend);
    int b = 0;
    CloudGrid g = grids[0];
    for (int64_t it = ibeg + wave; it < iend; it += 4) {
        const int64_t q = qorder ? (int64_t)qorder[it] : it;
        if (q < g.q_base || q >= g.q_base + g.q_len) {
            b = find_cloud_q(grids, nb, q);
            g = grids[b];
        }
        const float qx = queries[3 * q], qy = queries[3 * q + 1], qz = queries[3 * q + 2];
        int cnt = 0;
        if (g.s_len > 0) {
            for_each_candidate(g, qx, qy, qz, cell_start, sorted, lane, [&](const float4& c, bool active) {
                const bool hit = active && ref_d2(qx, qy, qz, c) < r2;
                cnt += __builtin_popcountll(__ballot(hit));
            });
        }
        if (lane == 0 && cnt < hist_n) atomicAdd(&nb_hist_bins[cnt], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < hist_n; i += 256) {
        const int v = nb_hist_bins[i];
        if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
}

template <int CAP, typename OutT>
__global__ __launch_bounds__(256) void nb_fill_kernel(const float* __restrict__ queries, int64_t nq,
                                                       const CloudGrid* __restrict__ grids, int nb,
                                                       const int32_t* __restrict__ cell_start,
                                                       const float4* __restrict__ sorted, float r2, int64_t ns,
                                                       int width, const int32_t* __restrict__ qorder, OutT* __restrict__ out,
                                                       int32_t* __restrict__ counts, int32_t* __restrict__ max_count,
                                                       unsigned long long* __restrict__ key_last)
{
    __shared__ unsigned long long slab_all[4][CAP];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    unsigned long long* slab = slab_all[wave];
    int local_max = 0;
    int64_t ibeg, iend;
    ws_block_range(nq, ibeg, iend);
    for (int64_t it = ibeg + wave; it < iend; it += 4) {
        const int64_t q = qorder ? (int64_t)qorder[it] : it;
        const int b = find_cloud_q(grids, nb, q);
        const CloudGrid g = grids[b];
        const float qx = queries[3 * q], qy = queries[3 * q + 1], qz = queries[3 * q + 2];
        int cnt = 0;
        if (g.s_len > 0) {
            for_each_candidate(g, qx, qy, qz, cell_start, sorted, lane, [&](const float4& c, bool active) {
                const float d2 = ref_d2(qx, qy, qz, c);
                const bool hit = active && d2 < r2;
                const unsigned long long m = __ballot(hit);
                if (hit) {
                    const int pos = cnt + __builtin_popcountll(m & ((1ull << lane) - 1ull));
                    if (pos < CAP)
                        slab[pos] = nb_key(d2, (unsigned)__float_as_int(c.w));
                }
                cnt += __builtin_popcountll(m);
            });
        }
        if (counts) {      // fused search: the true count (may exceed CAP -> the host reruns wider)
            if (lane == 0) counts[q] = cnt;
            local_max = max(local_max, cnt);
        }
        cnt = min(cnt, CAP);
        int m = 64;
        while (m < cnt) m <<= 1;
        for (int i = cnt + lane; i < m; i += 64) slab[i] = ~0ull;
        wave_lds_sync();
        if (cnt > 1) {
            for (int k = 2; k <= m; k <<= 1) {
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int t = lane; t < (m >> 1); t += 64) {
                        // t-th compare-exchange of this stage: insert a 0 bit at position log2(j)
                        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                        const int l = i | j;
                        const unsigned long long a = slab[i], bb = slab[l];
                        const bool up = (i & k) == 0;
                        if ((a > bb) == up) { slab[i] = bb; slab[l] = a; }
                    }
                    wave_lds_sync();
                }
            }
        }
        for (int j = lane; j < width; j += 64)
            out[q * width + j] = j < cnt ? (OutT)nb_key_index(slab[j]) : (OutT)ns;
        // key of the last neighbour kept when the row is truncated, "infinity" when every neighbour is kept
        if (key_last && lane == 0) key_last[q] = cnt > width ? slab[width - 1] : ~0ull;
        wave_lds_sync();
    }
    if (max_count) nb_publish_max(max_count, local_max, lane);
}

// Fast path for rows of at most 128 neighbours (every layer of the KP-FCNN pyramids):
//  * the 9 cell runs of the 3x3x3 block are resolved first (scalar loads of the 18 run bounds) and
//    their first 64 candidates fetched together, so nine independent gathers are in flight instead
//    of nine dependent round trips;
//  * hits are compacted through the wave's LDS slab, then each lane takes two keys (i and i+64) and
//    finds their sorted positions by counting the smaller keys of the lower distance buckets and of its own.
template <typename OutT>
__global__ __launch_bounds__(256) void nb_fill128_kernel(const float* __restrict__ queries, int64_t nq,
                                                          const CloudGrid* __restrict__ grids, int nb,
                                                          const int32_t* __restrict__ cell_start,
                                                          const float4* __restrict__ sorted, float r2, int64_t ns,
                                                          int width, const int32_t* __restrict__ qorder, OutT* __restrict__ out,
                                                          int32_t* __restrict__ counts, int32_t* __restrict__ max_count,
                                                          unsigned long long* __restrict__ key_last)
{
    constexpr int CAP = 128;
    __shared__ unsigned long long slab_all[4][CAP + 64];      // + one dummy slot per lane (unconditional writes)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    unsigned long long* slab = slab_all[wave];
    int local_max = 0;
    int64_t ibeg, iend;
    ws_block_range(nq, ibeg, iend);
    // queries come cloud by cloud (stacked order, and the cell order of self-queries follows the clouds'
    // cell ranges), so the element index only ever advances: keep it and its grid in registers
    int b = 0;
    CloudGrid g = grids[0];
    for (int64_t it = ibeg + wave; it < iend; it += 4) {
        const int64_t q = qorder ? (int64_t)qorder[it] : it;
        if (q < g.q_base || q >= g.q_base + g.q_len) {
            b = find_cloud_q(grids, nb, q);
            g = grids[b];
        }
        const float qx = queries[3 * q], qy = queries[3 * q + 1], qz = queries[3 * q + 2];
        int cnt = 0;
        auto take = [&](const float4& c, bool active) {
            const float d2 = ref_d2(qx, qy, qz, c);
            const int2 put = slab_compact(active && d2 < r2, CAP, lane, cnt);
            slab[put.x] = nb_key(d2, (unsigned)__float_as_int(c.w));
            cnt = put.y;
        };
        if (g.s_len > 0) {
            grid_walk(g, qx, qy, qz, cell_start, sorted, lane, take);
        }
        if (counts) {
            if (lane == 0) counts[q] = cnt;
            local_max = max(local_max, cnt);
        }
        cnt = min(cnt, CAP);
        wave_lds_sync();
        const unsigned long long a = lane < cnt ? slab[lane] : ~0ull;
        const unsigned long long bkey = lane + 64 < cnt ? slab[lane + 64] : ~0ull;
        // rank: the keys are distinct (the index is part of the key), so the number of smaller keys IS the sorted position.
        // One level of buckets in front of the counting (as in nb_fill_wide_kernel): 64 buckets over [0, r^2),
        // bucket = (int)(d2 * 64 / r^2) is monotone in d2, so rank = keys in smaller buckets + smaller keys of the own
        // bucket -- ~1 key per bucket: a 64-wide scan and a two- or three-step count instead of cnt (60 .. 90) steps
        __shared__ int hist_all[4][64];
        __shared__ unsigned char member_all[4][128];
        int* hist = hist_all[wave];
        unsigned char* member = member_all[wave];
        hist[lane] = 0;
        wave_lds_sync();
        const float bscale = 64.0f / r2;
        const int ba = min(63, (int)(nb_key_d2(a) * bscale));
        const int bb = min(63, (int)(nb_key_d2(bkey) * bscale));
        int pa = 0, pb = 0;
        if (lane < cnt) pa = atomicAdd(&hist[ba], 1);
        if (lane + 64 < cnt) pb = atomicAdd(&hist[bb], 1);
        wave_lds_sync();
        const int own = hist[lane];
        int incl = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            incl += lane >= o ? t : 0;
        }
        int maxb = own;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) maxb = max(maxb, __shfl_xor(maxb, o, 64));
        maxb = __builtin_amdgcn_readfirstlane(maxb);
        __shared__ int start_all[4][64];
        int* start = start_all[wave];
        start[lane] = incl - own;
        wave_lds_sync();
        const int sa = start[ba], sb = start[bb];
        const int na = lane < cnt ? hist[ba] : 0, nbk = lane + 64 < cnt ? hist[bb] : 0;
        if (lane < cnt) member[sa + pa] = (unsigned char)lane;
        if (lane + 64 < cnt) member[sb + pb] = (unsigned char)(lane + 64);
        wave_lds_sync();
        int ra = sa, rb = sb;
        for (int t = 0; t < maxb; ++t) {
            const bool oka = t < na, okb = t < nbk;
            const unsigned long long ka = slab[member[oka ? sa + t : 0]];
            const unsigned long long kb = slab[member[okb ? sb + t : 0]];
            ra += (oka && ka < a) ? 1 : 0;
            rb += (okb && kb < bkey) ? 1 : 0;
        }
        OutT* orow = out + q * width;
        if (lane < cnt && ra < width) orow[ra] = (OutT)nb_key_index(a);
        if (lane + 64 < cnt && rb < width) orow[rb] = (OutT)nb_key_index(bkey);
        for (int j = cnt + lane; j < width; j += 64) orow[j] = (OutT)ns;
        if (key_last) {     // the key at sorted position width-1 of a truncated row, "infinity" otherwise
            if (cnt > width) {
                if (lane < cnt && ra == width - 1) key_last[q] = a;
                if (lane + 64 < cnt && rb == width - 1) key_last[q] = bkey;
            } else if (lane == 0) {
                key_last[q] = ~0ull;
            }
        }
        wave_lds_sync();
    }
    if (max_count) nb_publish_max(max_count, local_max, lane);
}

// Nearest neighbour only: column 0 of the row the full search would write (the smallest (d2, index) key inside the radius),
// or ns.  What KP-FCNN reads of an UPSAMPLING matrix (closest_pool / nearest upsampling: models/blocks.py:80-92 take
// inds[:, 0]) -- without the compaction and the sort of a 60 .. 550-entry row.  Opt-in (ws_radius_neighbors_nearest_async).
template <typename OutT>
__global__ __launch_bounds__(256) void nb_nearest_kernel(const float* __restrict__ queries, int64_t nq,
                                                          const CloudGrid* __restrict__ grids, int nb,
                                                          const int32_t* __restrict__ cell_start,
                                                          const float4* __restrict__ sorted, float r2, int64_t ns,
                                                          const int32_t* __restrict__ qorder, OutT* __restrict__ out,
                                                          int32_t* __restrict__ any_hit)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    int64_t ibeg, iend;
    ws_block_range(nq, ibeg, iend);
    int b = 0;
    CloudGrid g = grids[0];
    int found_any = 0;
    for (int64_t it = ibeg + wave; it < iend; it += 4) {
        const int64_t q = qorder ? (int64_t)qorder[it] : it;
        if (q < g.q_base || q >= g.q_base + g.q_len) {
            b = find_cloud_q(grids, nb, q);
            g = grids[b];
        }
        const float qx = queries[3 * q], qy = queries[3 * q + 1], qz = queries[3 * q + 2];
        unsigned long long best = ~0ull;
        if (g.s_len > 0) {
            const CellRuns u = grid_cell_runs(g, qx, qy, qz, cell_start);      // grid_walk (ws_grid.h) spelt out: see there
            float4 c[9];
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                const int p = u.rb[r] + lane;
                c[r] = sorted[p < u.re[r] ? p : 0];
            }
            auto take = [&](const float4& cc, bool active) {
                const float d2 = ref_d2(qx, qy, qz, cc);
                const unsigned long long key = nb_key(d2, (unsigned)__float_as_int(cc.w));
                if (active && d2 < r2 && key < best) best = key;
            };
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                take(c[r], u.rb[r] + lane < u.re[r]);
                for (int p0 = u.rb[r] + 64; p0 < u.re[r]; p0 += 64) {
                    const int p = p0 + lane;
                    float4 cc = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (p < u.re[r]) cc = sorted[p];
                    take(cc, p < u.re[r]);
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o, 64);
            best = other < best ? other : best;
        }
        const unsigned first = nb_key_index(best);
        if (lane == 0) out[q] = best != ~0ull ? (OutT)first : (OutT)ns;
        found_any |= best != ~0ull ? 1 : 0;
    }
    if (any_hit && lane == 0 && found_any) nb_publish_max(any_hit, 1, 0);
}

// Rows of 129 .. 1024 neighbours: the deformable radius of BASELINE config 5 (datasets/common.py:500-502: every level is
// searched at 2 r, about 8 x the neighbours; calibrated limits 422 / 519 / 472).  Same candidate walk as nb_fill128; what
// changes is the sort.  Rank by counting is quadratic (500 keys: 250 000 comparisons per query) and the bitonic network
// of nb_fill_kernel<2048> runs 45 dependent LDS stages on a 64 KB slab (2 waves per SIMD): 4.2 ms per launch in round 2,
// 55 ms per config-5 step.  Here the keys go through ONE level of buckets first:
//   bucket(key) = min(NB - 1, (int)(d2 * NB / r^2))      -- monotone in d2 (a float multiply by a positive constant and
//                                                           the conversion both are), equal d2 share a bucket
//   rank(key)   = #keys in smaller buckets + #keys of the same bucket that are smaller
// so the sorted position is still a pure function of the (distinct) keys -- the LDS atomics below only hand out arbitrary
// slots INSIDE a bucket, which the final within-bucket count makes irrelevant: bit-identical rows from run to run.
// With NB = 256 a 500-key row has ~2 keys per bucket (~8 in the fullest): the within-bucket count is a handful of LDS
// reads per key, taken for all of a lane's keys together (independent chains).
template <typename OutT, int CAP>
__global__ __launch_bounds__(256) void nb_fill_wide_kernel(const float* __restrict__ queries, int64_t nq,
                                                           const CloudGrid* __restrict__ grids, int nb,
                                                           const int32_t* __restrict__ cell_start,
                                                           const float4* __restrict__ sorted, float r2, int64_t ns,
                                                           int width, const int32_t* __restrict__ qorder, OutT* __restrict__ out,
                                                           int32_t* __restrict__ counts, int32_t* __restrict__ max_count,
                                                           unsigned long long* __restrict__ key_last)
{
    constexpr int NB = 256, KPL = CAP / 64;       // CAP = 576 / 704 / 1024 keys per query: 8.3 / 9.5 / 12.7 KB of LDS per wave = 4 / 4 / 3 workgroups per CU
    __shared__ unsigned long long slab_all[4][CAP + 64];      // keys in arrival order (+ one dummy slot per lane)
    __shared__ unsigned short member_all[4][CAP];             // slab positions grouped by bucket
    __shared__ int hist_all[4][NB];
    __shared__ int start_all[4][NB];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    unsigned long long* slab = slab_all[wave];
    unsigned short* member = member_all[wave];
    int* hist = hist_all[wave];
    int* start = start_all[wave];
    const float bscale = (float)NB / r2;
    int local_max = 0;
    int64_t ibeg, iend;
    ws_block_range(nq, ibeg, iend);
    int b = 0;
    CloudGrid g = grids[0];
    for (int64_t it = ibeg + wave; it < iend; it += 4) {
        const int64_t q = qorder ? (int64_t)qorder[it] : it;
        if (q < g.q_base || q >= g.q_base + g.q_len) {
            b = find_cloud_q(grids, nb, q);
            g = grids[b];
        }
        const float qx = queries[3 * q], qy = queries[3 * q + 1], qz = queries[3 * q + 2];
        int cnt = 0;
        auto take = [&](const float4& c, bool active) {
            const float d2 = ref_d2(qx, qy, qz, c);
            const unsigned long long key = nb_key(d2, (unsigned)__float_as_int(c.w));      // (ahead of the ballot here, behind it in
            const int2 put = slab_compact(active && d2 < r2, CAP, lane, cnt);              //  nb_fill128_kernel: the orders the two schedules keep)
            slab[put.x] = key;
            cnt = put.y;
        };
        for (int i = lane; i < NB; i += 64) hist[i] = 0;
        if (g.s_len > 0) {
            // (the runs come one by one: through the CellRuns copy the 1024-key instantiations are scheduled differently)
            const CellBlock k = grid_cell_block(g, qx, qy, qz);
            int rb[9], re[9];
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                const int2 run = grid_cell_run(g, k, r, cell_start);
                rb[r] = run.x;
                re[r] = run.y;
            }
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                // runs of a few hundred candidates: two batches of 64 in flight per iteration
                for (int p0 = rb[r]; p0 < re[r]; p0 += 128) {
                    const int pa = p0 + lane, pb = p0 + 64 + lane;
                    const float4 ca = sorted[pa < re[r] ? pa : rb[r]];
                    const float4 cb = sorted[pb < re[r] ? pb : rb[r]];
                    take(ca, pa < re[r]);
                    if (p0 + 64 < re[r]) take(cb, pb < re[r]);
                }
            }
        }
        if (counts) {
            if (lane == 0) counts[q] = cnt;
            local_max = max(local_max, cnt);
        }
        const int cntc = min(cnt, CAP);
        wave_lds_sync();
        // ---- A: bucket of every key, slot inside the bucket from an LDS atomic
        unsigned long long key[KPL];
        int bk[KPL], pk[KPL];
#pragma unroll
        for (int j = 0; j < KPL; ++j) {
            key[j] = ~0ull; bk[j] = 0; pk[j] = 0;
            if (64 * j < cntc) {
                const int i = lane + 64 * j;
                if (i < cntc) {
                    key[j] = slab[i];
                    const float d2 = nb_key_d2(key[j]);
                    bk[j] = min(NB - 1, (int)(d2 * bscale));
                    pk[j] = atomicAdd(&hist[bk[j]], 1);
                }
            }
        }
        wave_lds_sync();
        // ---- B: exclusive scan of the histogram (lane owns 4 consecutive buckets), largest bucket
        const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
        const int own = (h0 + h1) + (h2 + h3);
        int incl = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            incl += lane >= o ? t : 0;
        }
        const int excl = incl - own;
        start[4 * lane] = excl; start[4 * lane + 1] = excl + h0; start[4 * lane + 2] = excl + h0 + h1; start[4 * lane + 3] = excl + h0 + h1 + h2;
        int maxb = max(max(h0, h1), max(h2, h3));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) maxb = max(maxb, __shfl_xor(maxb, o, 64));
        maxb = __builtin_amdgcn_readfirstlane(maxb);
        wave_lds_sync();
        // ---- C: slab positions grouped by bucket
        int sb[KPL], nbk[KPL];
#pragma unroll
        for (int j = 0; j < KPL; ++j) {
            sb[j] = 0; nbk[j] = 0;
            if (64 * j < cntc) {
                const int i = lane + 64 * j;
                if (i < cntc) {
                    sb[j] = start[bk[j]];
                    nbk[j] = hist[bk[j]];
                    member[sb[j] + pk[j]] = (unsigned short)i;
                }
            }
        }
        wave_lds_sync();
        // ---- D: sorted position = keys in smaller buckets + smaller keys of the own bucket
        int rank[KPL];
#pragma unroll
        for (int j = 0; j < KPL; ++j) rank[j] = sb[j];
        for (int t = 0; t < maxb; ++t) {
#pragma unroll
            for (int j = 0; j < KPL; ++j) {
                if (64 * j < cntc) {
                    const bool ok = t < nbk[j];
                    const unsigned long long other = slab[member[ok ? sb[j] + t : 0]];
                    rank[j] += (ok && other < key[j]) ? 1 : 0;
                }
            }
        }
        OutT* orow = out + q * width;
#pragma unroll
        for (int j = 0; j < KPL; ++j) {
            if (64 * j < cntc) {
                const int i = lane + 64 * j;
                if (i < cntc && rank[j] < width) orow[rank[j]] = (OutT)nb_key_index(key[j]);
                if (key_last && cnt > width && i < cntc && rank[j] == width - 1) key_last[q] = key[j];
            }
        }
        for (int j = cntc + lane; j < width; j += 64) orow[j] = (OutT)ns;
        if (key_last && cnt <= width && lane == 0) key_last[q] = ~0ull;
        wave_lds_sync();
    }
    if (max_count) nb_publish_max(max_count, local_max, lane);
}

// The bin fill hands out slots inside a cell through an atomic cursor (arrival order).  One thread per entry: its place
// among the entries of its cell by support index (rank by counting over the cell's few entries), written to the final copy.
// The cell-sorted copy, the cell order and the summation order of the grid-walk backward then are functions of the input alone.
__global__ __launch_bounds__(256) void nb_cell_rank_kernel(const float4* __restrict__ arrived, int64_t ns,
                                                            const int32_t* __restrict__ cell_of,
                                                            const int32_t* __restrict__ cell_start, float4* __restrict__ sorted)
{
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < ns; p += (int64_t)gridDim.x * 256) {
        const float4 v = arrived[p];
        const int idx = __float_as_int(v.w);
        const int c = cell_of[idx];
        const int beg = cell_start[c], end = cell_start[c + 1];
        int rank = 0;
        for (int j = beg; j < end; ++j) rank += __float_as_int(arrived[j].w) < idx ? 1 : 0;
        sorted[beg + rank] = v;
    }
}

__global__ __launch_bounds__(256) void nb_order_kernel(const float4* __restrict__ sorted, int64_t ns, int32_t* __restrict__ order)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < ns; i += (int64_t)gridDim.x * 256)
        order[i] = __float_as_int(sorted[i].w);
}

}  // namespace
