// weasal_amd/csrc/kpconv_bwd_grid_kernels.h -- KPConv gather backward w.r.t. x without a transposed table, gfx950 (wave64), and its
// launch per kernel size.  The slab template is the largest of the gather's families (80 instantiations at K = 15), so each
// kernel size is a unit of its own: kpconv_bwd_grid.hip (K = 15, and the launcher the entries call), kpconv_bwd_grid_k9.hip,
// kpconv_bwd_grid_k13.hip.  Each includes this header and instantiates launch_bwd_x_grid_k for its size.
//
// K4G  the sum of K4 (kpconv_bwd_x.hip) for self-query layers, the incoming pairs of a support re-derived from the cell grid
// of the neighbour search.  Here the slab form for rows up to 128 (kpconv_gather_bwd_x_grid_kernel); the queue form for any
// in-degree is in kpconv_bwd_gridw.hip (a unit of its own for the compile time: the two templates hold 102 of the gather's
// 257 instantiations).  The entry pool and its list phase are in kpconv_device.h.
#pragma once
#include "kpconv_launch.h"
#include "ws_dispatch.h"

namespace {

// ---------------------------------------------------------------------------------------------
// K4 without a transposed table (self-query layers: q_pts == s_pts, the same cloud on both sides).
// The pairs that reach support s are re-derived from the cell grid the neighbour search built:
//   q -> s is a pair  <=>  d2(q, s) < r^2  and  (d2(q, s), s) <= key_last[q],
// key_last[q] being the (distance, index) key of the last neighbour K1 kept in q's row ("infinity" for a
// row that was not truncated).  The distance is symmetric bit for bit (ws_grid.h: ref_d2), so the wave of s
// walks the 3x3x3 cell block exactly as K1 does, keeps the candidates that pass the membership test, orders
// them by index (= ascending pair id, the order of the transposed table, so the sums are the same bits) and
// runs K4's list / flush on them.  No counting-sort atomics, no scattered fill, no per-list sort: the
// table build of the big level-0 matrix (1.6 ms per step) disappears.
// ---------------------------------------------------------------------------------------------
constexpr int GRID_SLAB = 192;      // incoming pairs per support (the search reports rows up to 128)

template <int K, int G, int MODE, bool VEC, typename T = float, bool SORT = true>
__global__ __launch_bounds__(256) void kpconv_gather_bwd_x_grid_kernel(
    const float* __restrict__ s_pts, int64_t ns, const CloudGrid* __restrict__ grids, int nb,
    const int32_t* __restrict__ cell_start, const float4* __restrict__ sorted,
    const unsigned long long* __restrict__ key_last, float r2, const T* __restrict__ dwf, int ci,
    const float* __restrict__ kernel_points, const float* __restrict__ deformed_kp, const float* __restrict__ modulations,
    GeomParams g, T* __restrict__ dx, const int32_t* __restrict__ order, int32_t* __restrict__ overflow)
{
    constexpr int CC = 4 * G;
    constexpr int S = 64 / G;
    constexpr int EPL = GRID_SLAB / 64;          // slab entries per lane
    __shared__ uint2 pool_all[4][POOL_ALLOC];
    __shared__ int segs_all[4][K + 1];
    __shared__ float4 slab_all[4][GRID_SLAB + 64];      // + one dummy slot per lane (unconditional writes)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    uint2* pool = pool_all[wave];
    int* segs = segs_all[wave];
    float4* slab = slab_all[wave];
    const int j = lane % G;
    const int slot = lane / G;
    const float inv_extent = 1.0f / g.extent;

    float kpr[MODE == 0 ? 3 * K : 1];
    if (MODE == 0) {
#pragma unroll
        for (int t = 0; t < 3 * K; ++t) kpr[t] = kernel_points[t];
    }

    int64_t item0, istep, iend;
    ws_wave_items(ns, order ? g.ilv : 0, wave, item0, istep, iend);
    CloudGrid gr = grids[0];        // supports come cloud by cloud: the element's grid stays in registers
    for (int64_t item = item0; item < iend; item += istep) {
        const int64_t s = order ? (int64_t)order[item] : item;
        if (s < gr.s_base || s >= gr.s_base + gr.s_len) {
            int b = 0;
            while (b + 1 < nb && s >= grids[b].s_base + grids[b].s_len) ++b;
            gr = grids[b];
        }
        const float sx = s_pts[3 * s + 0], sy = s_pts[3 * s + 1], sz = s_pts[3 * s + 2];
        // ---- candidates: the 9 cell runs around s, membership test, compaction into the slab
        int cnt = 0;
        auto take = [&](const float4& c, bool active) {
            // K1 evaluated this pair with c as the query and s as the support: diff = query - support
            const float d2 = ref_d2(c.x, c.y, c.z, make_float4(sx, sy, sz, 0.0f));
            const unsigned long long key = nb_key(d2, (unsigned)s);
            bool hit = active && d2 < r2;
            hit = hit && key <= key_last[hit ? __float_as_int(c.w) : 0];          // unconditional gather
            const int2 put = slab_compact(hit, GRID_SLAB, lane, cnt);
            slab[put.x] = c;
            cnt = put.y;
        };
        // a support with an untruncated row of its own: every point within the radius is in that row (the distance is
        // symmetric bit for bit), so the queries that kept s are among its entries -- ~60 candidates instead of the ~700 of
        // the 27-cell walk.  Wave-uniform branch (s is).
        const bool from_row = g.rows != nullptr && key_last[s] == ~0ull;
        if (from_row) {
            for (int h0 = 0; h0 < g.rows_h; h0 += 64) {
                const int col = h0 + lane;
                const int64_t qi = col < g.rows_h ? g.rows[s * g.rows_h + col] : -1;
                const bool active = qi >= 0 && qi < ns;
                const int64_t qq = active ? qi : 0;
                take(make_float4(s_pts[3 * qq + 0], s_pts[3 * qq + 1], s_pts[3 * qq + 2], __int_as_float((int)qq)), active);
            }
        } else if (gr.s_len > 0) {
            const CellRuns u = grid_cell_runs(gr, sx, sy, sz, cell_start);      // grid_walk (ws_grid.h) spelt out: see there
            float4 c[9];
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                const int p = u.rb[r] + lane;
                c[r] = sorted[p < u.re[r] ? p : 0];          // unconditional, masked by `active`
            }
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
        if (cnt > GRID_SLAB) {      // cannot happen when the search reported rows <= 128; flagged, never silent
            if (lane == 0) atomicMax(overflow, cnt);
            cnt = GRID_SLAB;
        }
        wave_lds_sync();
        // ---- order by index: rank by counting (distinct indices), then permute through registers; only as many
        //      entries per lane as the in-degree needs (1 for <= 64 incoming pairs).  SORT = false keeps the order of the
        //      grid walk (cell run by cell run, compaction order inside a batch of 64): just as deterministic -- it depends
        //      on the grid only -- but not the pair order of the transposed table, so dx then agrees with K4 to fp32
        //      re-association (1e-6) instead of bit for bit; the counting loop it skips is ~ a third of this kernel's
        //      instructions (the kernel is issue-bound: DESIGN.md section 4)
        if (SORT) {
            float4 e[EPL];
            int rk[EPL];
#pragma unroll
            for (int u = 0; u < EPL; ++u) {
                e[u] = lane + 64 * u < cnt ? slab[lane + 64 * u] : make_float4(0.f, 0.f, 0.f, __int_as_float(0x7fffffff));
                rk[u] = 0;
            }
            if (cnt <= 64) {
                for (int i = 0; i < cnt; ++i) rk[0] += __float_as_int(slab[i].w) < __float_as_int(e[0].w) ? 1 : 0;
            } else if (cnt <= 128) {
                for (int i = 0; i < cnt; ++i) {
                    const int ki = __float_as_int(slab[i].w);
                    rk[0] += ki < __float_as_int(e[0].w) ? 1 : 0;
                    rk[1] += ki < __float_as_int(e[1].w) ? 1 : 0;
                }
            } else {
                for (int i = 0; i < cnt; ++i) {
                    const int ki = __float_as_int(slab[i].w);
#pragma unroll
                    for (int u = 0; u < EPL; ++u) rk[u] += ki < __float_as_int(e[u].w) ? 1 : 0;
                }
            }
            wave_lds_sync();
#pragma unroll
            for (int u = 0; u < EPL; ++u)
                if (lane + 64 * u < cnt) slab[rk[u]] = e[u];
            wave_lds_sync();
        }
        // ---- K4's list / flush over the slab
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
            for (int p0 = 0; p0 < cnt; p0 += 64) {
                const int p = p0 + lane;
                const bool real = p < cnt;
                const float4 c = real ? slab[p] : make_float4(0.f, 0.f, 0.f, 0.f);
                const int q = real ? __float_as_int(c.w) : 0;
                const float nx = sx - c.x, ny = sy - c.y, nz = sz - c.z;
                const float* lkp = deformed_kp ? deformed_kp + (int64_t)q * (3 * K) : kernel_points;
                const float* lmod = modulations ? modulations + (int64_t)q * K : nullptr;
                auto kp = [&](int k, int cidx) { return MODE == 0 ? kpr[MODE == 0 ? 3 * k + cidx : 0] : lkp[3 * k + cidx]; };
                auto nomin = [&](int, float) {};
                int total = 0, maxlen = 0;
                kp_list<K, MODE>(nx, ny, nz, real, kp, g, inv_extent, (unsigned)(q * K), 1u, lmod, pool, segs, lane, total,
                                 maxlen, nomin);
                if (total <= POOL) {
                    flush(total);
                } else {
                    for (int sub = 0; sub < 4; ++sub) {
                        total = 0; maxlen = 0;
                        kp_list<K, MODE>(nx, ny, nz, real && (lane >> 4) == sub, kp, g, inv_extent, (unsigned)(q * K), 1u, lmod,
                                         pool, segs, lane, total, maxlen, nomin);
                        flush(total);
                    }
                }
            }
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
        wave_lds_sync();
    }
}

}  // namespace

namespace kpconv {

// kpconv_gather_bwd_x_grid_kernel<KN, ...> for ws_kpconv_gather_bwd_x_grid / _bf16 / _gated; bf16 rows are VEC only, and K = 15 only
template <int KN>
void launch_bwd_x_grid_k(const GatherPlan& p, void* stream, const float* s_pts, int64_t ns, const GridView& v, int32_t nb, const void* dwf,
                         int32_t ci, const float* kernel_points, const float* deformed_kp, const float* modulations, const GeomParams& g,
                         void* dx, const int32_t* order, int32_t* overflow)
{
    dispatch([&](auto bf, auto gr, auto md, auto vec, auto sort) {
        using T = Row<bf.value>;
        if constexpr ((!bf.value || vec.value) && (KN == 15 || !bf.value))
            kpconv_gather_bwd_x_grid_kernel<KN, gr.value, md.value, vec.value != 0, T, sort.value != 0><<<p.grid, 256, 0, (hipStream_t)stream>>>(
                s_pts, ns, v.grids, nb, v.cell_start, v.sorted, v.key_last, v.r2, (const T*)dwf, ci, kernel_points, deformed_kp, modulations, g,
                (T*)dx, order, overflow);
    }, Flag{p.bf16}, Pick<1, 2, 4, 8, 16>{p.n}, Pick<0, 1>{p.mode}, Flag{p.vec}, Flag{p.sort});
}
// the unit of size KN
#define WS_BWD_X_GRID_UNIT(KN)                                                                                                        \
    template void launch_bwd_x_grid_k<KN>(const GatherPlan&, void*, const float*, int64_t, const GridView&, int32_t, const void*, int32_t, \
                                          const float*, const float*, const float*, const GeomParams&, void*, const int32_t*, int32_t*);

}  // namespace kpconv
