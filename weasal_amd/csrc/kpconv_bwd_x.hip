// weasal_amd/csrc/kpconv_bwd_x.hip -- KPConv gather backward w.r.t. x through the transposed table, gfx950 (wave64), and its launches.
//
// K4  kpconv_gather_bwd_x : dx[s,c] = sum_{(q,h)->s} sum_k w * dwf[q,k,c]   (transposed table, no atomics)
// One support per wave (kpconv_gather_bwd_x_kernel) or four (kpconv_gather_bwd_x_packed_kernel); the entry pool and its list
// phase are in kpconv_device.h.  The table-free form of the same sum is in kpconv_bwd_grid.hip.
#include "kpconv_launch.h"
#include "ws_dispatch.h"

namespace {

// ---------------------------------------------------------------------------------------------
// K4 backward w.r.t. x through the transposed table: dx[s, :] = sum_e weight_e * dwf[row_e, :]
// with row_e = q*K + k.  One wave per support; the flush is balanced over the S slots
// (slot s takes entries [s*per, (s+1)*per)) and the S partial sums are combined by shuffles.
// ---------------------------------------------------------------------------------------------
// One support s by the whole wave: every 64-pair chunk of its table segment listed and flushed, per channel chunk.  The body
// of kpconv_gather_bwd_x_kernel, shared with the packed form below (its path for a support that does not fit a lane group).
// kpr: the rigid kernel points (MODE 0), wave-uniform.
template <int K, int G, int MODE, bool VEC, typename T>
__device__ __forceinline__ void bwd_x_support(
    int64_t s, const float* __restrict__ q_pts, const float* __restrict__ s_pts, int h, const int32_t* __restrict__ t_offsets,
    const int32_t* __restrict__ t_pairs, const T* __restrict__ dwf, int ci, const float* __restrict__ kernel_points,
    const float* __restrict__ deformed_kp, const float* __restrict__ modulations, const GeomParams& g, T* __restrict__ dx,
    const float (&kpr)[MODE == 0 ? 3 * K : 1], float inv_extent, uint2* pool, int* segs, int lane)
{
    constexpr int CC = 4 * G;
    constexpr int S = 64 / G;
    const int j = lane % G;
    const int slot = lane / G;
    {
        const float sx = s_pts[3 * s + 0], sy = s_pts[3 * s + 1], sz = s_pts[3 * s + 2];
        const int beg = t_offsets[s], end = t_offsets[s + 1];
        for (int cc0 = 0; cc0 < ci; cc0 += CC) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            const int ch = cc0 + 4 * j;
            const bool chok = VEC ? (ch + 3 < ci) : (ch < ci);
            const int chl = chok ? ch : 0;
            // the gate row (GeomParams::gate) is fetched here, ahead of the walk: at the store its latency has long passed
            float4 gq = make_float4(1.f, 1.f, 1.f, 1.f);
            if (g.gate && slot == 0) {
                const T* gy = reinterpret_cast<const T*>(g.gate) + s * ci + ch;
                if (VEC) {
                    if (chok) gq = ld4(gy);
                } else {
                    if (ch + 0 < ci) gq.x = ld1(gy + 0);
                    if (ch + 1 < ci) gq.y = ld1(gy + 1);
                    if (ch + 2 < ci) gq.z = ld1(gy + 2);
                    if (ch + 3 < ci) gq.w = ld1(gy + 3);
                }
            }
            auto flush = [&](int total) {
                wave_lds_sync();
                total = min(total, POOL);
                const int per = (total + S - 1) / S;
                const int lo = slot * per;
                const int hi = chok ? min(lo + per, total) : lo;
                for (int it = 0; it < per; it += 4) {
                    float4 v[4];
                    float w[4];
                    uint2 e[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        e[u] = pool[min(lo + it + u, POOL + 7)];
                        keep_unconditional(e[u]);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const bool ok = lo + it + u < hi;
                        e[u].x = ok ? e[u].x : 0u;
                        w[u] = ok ? __uint_as_float(e[u].y) : 0.0f;
                        v[u] = load_row_piece<VEC>(dwf, e[u].x, ci, chl);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        acc.x = fmaf(w[u], v[u].x, acc.x);
                        acc.y = fmaf(w[u], v[u].y, acc.y);
                        acc.z = fmaf(w[u], v[u].z, acc.z);
                        acc.w = fmaf(w[u], v[u].w, acc.w);
                    }
                }
                wave_lds_sync();
            };
            for (int p0 = beg; p0 < end; p0 += 64) {
                const int p = p0 + lane;
                const bool real = p < end;
                const int pair = real ? t_pairs[p] : 0;
                const int q = pair / h;
                const float nx = sx - q_pts[3 * (int64_t)q + 0];
                const float ny = sy - q_pts[3 * (int64_t)q + 1];
                const float nz = sz - q_pts[3 * (int64_t)q + 2];
                const float* lkp = deformed_kp ? deformed_kp + (int64_t)q * (3 * K) : kernel_points;   // per lane if deformed
                const float* lmod = modulations ? modulations + (int64_t)q * K : nullptr;
                auto kp = [&](int k, int c) { return MODE == 0 ? kpr[MODE == 0 ? 3 * k + c : 0] : lkp[3 * k + c]; };
                auto nomin = [&](int, float) {};
                int total = 0, maxlen = 0;
                if constexpr (MODE == 2) {
                    const float4* kq = g.kp4 + (int64_t)q * K;
                    kp_list_def<K>(nx, ny, nz, real, kq, inv_extent, (unsigned)(q * K), pool, segs, lane, total, maxlen);
                    if (total <= POOL) {
                        flush(total);
                    } else {
                        for (int sub = 0; sub < 4; ++sub) {
                            total = 0; maxlen = 0;
                            kp_list_def<K>(nx, ny, nz, real && (lane >> 4) == sub, kq, inv_extent, (unsigned)(q * K), pool, segs, lane,
                                           total, maxlen);
                            flush(total);
                        }
                    }
                    continue;
                }
                kp_list<K, MODE == 2 ? 1 : MODE>(nx, ny, nz, real, kp, g, inv_extent, (unsigned)(q * K), 1u, lmod, pool, segs, lane, total,
                                 maxlen, nomin);
                if (total <= POOL) {
                    flush(total);
                } else {
                    for (int sub = 0; sub < 4; ++sub) {
                        total = 0; maxlen = 0;
                        kp_list<K, MODE == 2 ? 1 : MODE>(nx, ny, nz, real && (lane >> 4) == sub, kp, g, inv_extent, (unsigned)(q * K), 1u, lmod,
                                         pool, segs, lane, total, maxlen, nomin);
                        flush(total);
                    }
                }
            }
            // sum the S slots
#pragma unroll
            for (int o = G; o < 64; o <<= 1) {
                acc.x += __shfl_xor(acc.x, o, 64);
                acc.y += __shfl_xor(acc.y, o, 64);
                acc.z += __shfl_xor(acc.z, o, 64);
                acc.w += __shfl_xor(acc.w, o, 64);
            }
            if (slot == 0) {
                T* dst = dx + s * ci + ch;
                if (g.gate) {
                    acc.x *= gq.x > 0.0f ? 1.0f : g.gate_slope; acc.y *= gq.y > 0.0f ? 1.0f : g.gate_slope;
                    acc.z *= gq.z > 0.0f ? 1.0f : g.gate_slope; acc.w *= gq.w > 0.0f ? 1.0f : g.gate_slope;
                }
                if (VEC) {
                    if (chok) st4(dst, acc);
                } else {
                    if (ch + 0 < ci) st1(dst + 0, acc.x);
                    if (ch + 1 < ci) st1(dst + 1, acc.y);
                    if (ch + 2 < ci) st1(dst + 2, acc.z);
                    if (ch + 3 < ci) st1(dst + 3, acc.w);
                }
            }
        }
    }
}

template <int K, int G, int MODE, bool VEC, typename T = float>
__global__ __launch_bounds__(256) void kpconv_gather_bwd_x_kernel(
    const float* __restrict__ q_pts, int64_t nq, const float* __restrict__ s_pts, int64_t ns,
    int h, const int32_t* __restrict__ t_offsets, const int32_t* __restrict__ t_pairs,
    const T* __restrict__ dwf, int ci, const float* __restrict__ kernel_points,
    const float* __restrict__ deformed_kp, const float* __restrict__ modulations, GeomParams g,
    T* __restrict__ dx, const int32_t* __restrict__ order)
{
    static_assert(K <= 16 && POOL >= 16 * K, "pool sizing");
    __shared__ uint2 pool_all[4][POOL_ALLOC];
    __shared__ int segs_all[4][K + 1];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    uint2* pool = pool_all[wave];
    int* segs = segs_all[wave];
    const float inv_extent = 1.0f / g.extent;

    float kpr[MODE == 0 ? 3 * K : 1];
    if (MODE == 0) {
#pragma unroll
        for (int t = 0; t < 3 * K; ++t) kpr[t] = kernel_points[t];
    }

    int64_t item0, istep, iend;
    ws_wave_items(ns, order ? g.ilv : 0, wave, item0, istep, iend);
    for (int64_t item = item0; item < iend; item += istep) {
        const int64_t s = order ? (int64_t)order[item] : item;
        bwd_x_support<K, G, MODE, VEC, T>(s, q_pts, s_pts, h, t_offsets, t_pairs, dwf, ci, kernel_points, deformed_kp, modulations, g, dx,
                                          kpr, inv_extent, pool, segs, lane);
    }
}

// ---------------------------------------------------------------------------------------------
// K4, packed: four supports per wave, for tables of few incoming pairs per support (the strided layers: nq * h / ns ~ 10).
// The list phase above costs the same for 10 live lanes as for 64; here the wave takes four consecutive items of its
// workgroup's range and lane 16 j + i lists pair i of support j, so one pass of the 15 kernel points serves four supports.
//   list    the influences by the expressions of kp_list (MODE 0); a live lane's rank is the number of live lanes below it
//           inside its 16-lane group, and each group fills its own quarter of the wave's pool -- kernel point major, pair
//           ascending: the entry order kpconv_gather_bwd_x_kernel produces for that support alone.
//   flush   a support owns 16 / G real slots; a real slot carries four of the S = 64 / G slots of the single-support kernel
//           (four accumulators, the four chains' loads in flight together), each chain its range of per = ceil(total / S)
//           entries in order.  The four are added as (a0 + a1) + (a2 + a3) and the real slots by the xor butterfly inside the
//           group: the association of the single-support kernel's butterfly, so every sum has its operands in its order.
//           A chain there ends with one to three weight-0 products with row 0 where per is no multiple of 4 (the padding of its
//           4-wide unroll).  They are kept, so that a NaN / infinity in row 0 or a negative-zero sum comes out with the same bits
//           too: fmaf(0, row0, a) applied once gives what applying it one to three times gives, so one product per chain does it.
//   ci > 4 G   the pool is built once per quad and flushed once per channel chunk.
// A support with more than 16 pairs, or whose entries overflow its quarter, goes through bwd_x_support after the quad's
// flush (wave-uniform branches); the groups past the end of the range are masked.  Rigid / linear / sum, float4 rows only.
// ---------------------------------------------------------------------------------------------
template <int K, int G, bool VEC, typename T = float>
__global__ __launch_bounds__(256) void kpconv_gather_bwd_x_packed_kernel(
    const float* __restrict__ q_pts, int64_t nq, const float* __restrict__ s_pts, int64_t ns,
    int h, const int32_t* __restrict__ t_offsets, const int32_t* __restrict__ t_pairs,
    const T* __restrict__ dwf, int ci, const float* __restrict__ kernel_points,
    const float* __restrict__ deformed_kp, const float* __restrict__ modulations, GeomParams g,
    T* __restrict__ dx, const int32_t* __restrict__ order)
{
    constexpr int CC = 4 * G;
    constexpr int S = 64 / G;          // slots of the single-support kernel: four per real slot here
    constexpr int QP = POOL / 4;       // pool entries of one group
    static_assert(VEC && G <= 16 && K <= 16 && POOL >= 16 * K, "float4 rows, a support per 16 lanes");
    __shared__ uint2 pool_all[4][POOL_ALLOC];
    __shared__ int segs_all[4][K + 1];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    uint2* pool = pool_all[wave];
    const int grp = lane >> 4, li = lane & 15;
    const int j = li % G;
    const int rslot = li / G;
    const unsigned gbase = (unsigned)(grp * QP), dummy = (unsigned)(POOL + 8 + lane);
    const unsigned below = (1u << li) - 1u;
    const float inv_extent = 1.0f / g.extent;

    float kpr[3 * K];
#pragma unroll
    for (int t = 0; t < 3 * K; ++t) kpr[t] = kernel_points[t];

    int64_t ibeg, iend;
    ws_block_range(ns, ibeg, iend);
    for (int64_t item = ibeg + 4 * wave; item < iend; item += 16) {
        const int64_t mine = item + grp;
        const bool have = mine < iend;
        const int64_t s = have ? (order ? (int64_t)order[mine] : mine) : 0;
        const int beg = have ? t_offsets[s] : 0, end = have ? t_offsets[s + 1] : 0;
        const bool fits16 = have && end - beg <= 16;
        // ---- list: lane = (support, pair)
        const bool real = fits16 && beg + li < end;
        const int pair = real ? t_pairs[beg + li] : 0;
        const int q = pair / h;
        float nx = 0.f, ny = 0.f, nz = 0.f;                    // (a lane without a pair reads no query: q_pts may be empty)
        if (real) {
            nx = s_pts[3 * s + 0] - q_pts[3 * (int64_t)q + 0];
            ny = s_pts[3 * s + 1] - q_pts[3 * (int64_t)q + 1];
            nz = s_pts[3 * s + 2] - q_pts[3 * (int64_t)q + 2];
        }
        int total = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float ex = nx - kpr[3 * k + 0], ey = ny - kpr[3 * k + 1], ez = nz - kpr[3 * k + 2];
            const float d = list_d2<K>(ex, ey, ez);                // (the expressions of kp_list: the same bits as the single-support form)
            float w = list_linear<K>(d, inv_extent);
            w = real ? w : 0.0f;
            const unsigned long long m = __ballot(w != 0.0f);
            const unsigned half = grp >= 2 ? (unsigned)(m >> 32) : (unsigned)m;
            const unsigned gm = (half >> (16 * (grp & 1))) & 0xffffu;         // the live lanes of this lane's group
            const unsigned pos = (unsigned)total + (unsigned)__builtin_popcount(gm & below);
            const bool ok = (w != 0.0f) && pos < (unsigned)QP;
            pool[ok ? gbase + pos : dummy] = make_uint2((unsigned)(q * K + k), __float_as_uint(w));
            total += __builtin_popcount(gm);
        }
        const bool packed = fits16 && total <= QP;                           // per group
        const unsigned long long single = __ballot(have && !packed && li == 0);   // bit 16 j: support j takes the whole wave
        total = packed ? total : 0;
        wave_lds_sync();
        // ---- flush: lane = (support, real slot, 16-byte piece)
        const int per = (total + S - 1) / S;
        for (int cc0 = 0; cc0 < ci; cc0 += CC) {
            const int ch = cc0 + 4 * j;
            const bool chok = ch + 3 < ci;
            const int chl = chok ? ch : 0;
            float4 gq = make_float4(1.f, 1.f, 1.f, 1.f);
            if (g.gate && rslot == 0 && packed && chok) gq = ld4(reinterpret_cast<const T*>(g.gate) + s * ci + ch);
            float4 pad = make_float4(0.f, 0.f, 0.f, 0.f);
            if (per & 3) pad = load_row_piece<VEC>(dwf, 0u, ci, chl);
            float4 a[4];
            int lo[4], hi[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                lo[u] = (4 * rslot + u) * per;
                hi[u] = chok ? min(lo[u] + per, total) : lo[u];
            }
            for (int it = 0; it < per; ++it) {
                float4 v[4];
                float w[4];
                uint2 e[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    e[u] = pool[gbase + (unsigned)min(lo[u] + it, QP - 1)];
                    keep_unconditional(e[u]);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool ok = lo[u] + it < hi[u];
                    e[u].x = ok ? e[u].x : 0u;
                    w[u] = ok ? __uint_as_float(e[u].y) : 0.0f;
                    v[u] = load_row_piece<VEC>(dwf, e[u].x, ci, chl);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    a[u].x = fmaf(w[u], v[u].x, a[u].x);
                    a[u].y = fmaf(w[u], v[u].y, a[u].y);
                    a[u].z = fmaf(w[u], v[u].z, a[u].z);
                    a[u].w = fmaf(w[u], v[u].w, a[u].w);
                }
            }
            if (per & 3) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    a[u].x = fmaf(0.0f, pad.x, a[u].x);
                    a[u].y = fmaf(0.0f, pad.y, a[u].y);
                    a[u].z = fmaf(0.0f, pad.z, a[u].z);
                    a[u].w = fmaf(0.0f, pad.w, a[u].w);
                }
            }
            float4 acc;
            acc.x = (a[0].x + a[1].x) + (a[2].x + a[3].x);
            acc.y = (a[0].y + a[1].y) + (a[2].y + a[3].y);
            acc.z = (a[0].z + a[1].z) + (a[2].z + a[3].z);
            acc.w = (a[0].w + a[1].w) + (a[2].w + a[3].w);
#pragma unroll
            for (int o = G; o < 16; o <<= 1) {
                acc.x += __shfl_xor(acc.x, o, 64);
                acc.y += __shfl_xor(acc.y, o, 64);
                acc.z += __shfl_xor(acc.z, o, 64);
                acc.w += __shfl_xor(acc.w, o, 64);
            }
            if (rslot == 0 && packed && chok) {
                if (g.gate) {
                    acc.x *= gq.x > 0.0f ? 1.0f : g.gate_slope; acc.y *= gq.y > 0.0f ? 1.0f : g.gate_slope;
                    acc.z *= gq.z > 0.0f ? 1.0f : g.gate_slope; acc.w *= gq.w > 0.0f ? 1.0f : g.gate_slope;
                }
                st4(dx + s * ci + ch, acc);
            }
        }
        wave_lds_sync();
        // ---- the supports that did not fit a group, one after the other with the whole wave
        if (single) {
#pragma unroll 1
            for (int t = 0; t < 4; ++t) {
                if ((single >> (16 * t)) & 1ull) {
                    const int64_t s1 = order ? (int64_t)order[item + t] : item + t;
                    bwd_x_support<K, G, 0, VEC, T>(s1, q_pts, s_pts, h, t_offsets, t_pairs, dwf, ci, kernel_points, nullptr, nullptr, g, dx,
                                                   kpr, inv_extent, pool, segs_all[wave], lane);
                }
            }
        }
    }
}

}  // namespace

namespace kpconv {

// kpconv_gather_bwd_x_kernel for ws_kpconv_gather_bwd_x* (MODE 0 / 1) and ws_kpconv_gather_bwd_x_def (MODE 2); bf16 rows are VEC only
void launch_bwd_x(const GatherPlan& p, void* stream, const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, int32_t h,
                  const int32_t* t_offsets, const int32_t* t_pairs, const void* dwf, int32_t ci, const float* kernel_points,
                  const float* deformed_kp, const float* modulations, const GeomParams& g, void* dx, const int32_t* order)
{
    dispatch([&](auto bf, auto gr, auto mode, auto vec, auto kn) {
        using T = Row<bf.value>;
        if constexpr ((!bf.value || vec.value) && (kn.value == 15 || (!bf.value && mode.value != 2)))
            kpconv_gather_bwd_x_kernel<kn.value, gr.value, mode.value, vec.value != 0, T><<<p.grid, 256, 0, (hipStream_t)stream>>>(
                q_pts, nq, s_pts, ns, h, t_offsets, t_pairs, (const T*)dwf, ci, kernel_points, deformed_kp, modulations, g, (T*)dx, order);
    }, Flag{p.bf16}, Pick<1, 2, 4, 8, 16>{p.n}, Pick<0, 1, 2>{p.mode}, Flag{p.vec}, Pick<WS_KP_SIZES>{p.k});
}

// kpconv_gather_bwd_x_packed_kernel for ws_kpconv_gather_bwd_x_packed: f32 float4 rows, MODE 0
void launch_bwd_x_packed(const GatherPlan& p, void* stream, const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, int32_t h,
                         const int32_t* t_offsets, const int32_t* t_pairs, const float* dwf, int32_t ci, const float* kernel_points,
                         const GeomParams& g, float* dx, const int32_t* order)
{
    dispatch([&](auto gr, auto kn) {
        kpconv_gather_bwd_x_packed_kernel<kn.value, gr.value, true, float><<<p.grid, 256, 0, (hipStream_t)stream>>>(
            q_pts, nq, s_pts, ns, h, t_offsets, t_pairs, dwf, ci, kernel_points, nullptr, nullptr, g, dx, order);
    }, Pick<1, 2, 4, 8, 16>{p.n}, Pick<WS_KP_SIZES>{p.k});
}

}  // namespace kpconv
