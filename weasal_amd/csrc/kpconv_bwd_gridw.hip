// weasal_amd/csrc/kpconv_bwd_gridw.hip -- the table-free KPConv gather backward w.r.t. x for wide rows, gfx950 (wave64), and its launches.
//
// K4G  as kpconv_bwd_grid.hip (the membership test is described there), with the slab as a queue: any in-degree
// (kpconv_gather_bwd_x_gridw_kernel), and kp4_rmax_kernel, the helper of its entry.  The entry pool and its list phase are
// in kpconv_device.h.
#include "kpconv_launch.h"
#include "ws_dispatch.h"

namespace {

// ---------------------------------------------------------------------------------------------
// K4G for wide rows: in-degrees of several hundred pairs per support (the deformable radius of BASELINE config 5:
// limits 422 / 519 / 472).  Same membership test as kpconv_gather_bwd_x_grid_kernel; what changes:
//   * the slab is a QUEUE, not a bound: whenever it holds 64 candidates more than one list phase consumes, the full
//     64-entry batches are run through the list / flush phases and the remainder moves to the front -- any in-degree,
//     no capacity flag, every list phase but the last on 64 live lanes;
//   * accumulators for up to NCH channel chunks live in registers, so the candidates are walked ONCE per support
//     whatever the row width (one pass for ci <= 4 G NCH = 256 channels);
//   * the candidate runs are walked by a rolled loop (run bounds in LDS): with ~300 candidates per run the first-batch
//     prefetch of the narrow kernel buys nothing and its nine-fold unrolled body would be inlined around every drain;
//   * MODE 2: the deformable fast path (kp_list_def).
// Summation order = order of the walk (a function of the grid alone): deterministic, equal to the transposed-table
// form up to fp32 re-association.
// ---------------------------------------------------------------------------------------------
template <int K, int G, int MODE, bool VEC, int NCH, typename T = float>
__global__ __launch_bounds__(256) void kpconv_gather_bwd_x_gridw_kernel(
    const float* __restrict__ s_pts, int64_t ns, const CloudGrid* __restrict__ grids, int nb,
    const int32_t* __restrict__ cell_start, const float4* __restrict__ sorted,
    const unsigned long long* __restrict__ key_last, float r2, const T* __restrict__ dwf, int ci,
    const float* __restrict__ kernel_points, const float* __restrict__ deformed_kp, const float* __restrict__ modulations,
    GeomParams g, T* __restrict__ dx, const int32_t* __restrict__ order)
{
    constexpr int CC = 4 * G;
    constexpr int S = 64 / G;
    static_assert(NCH == 1 || NCH == 2 || NCH == 4, "channel chunks whose accumulators stay in registers");
    constexpr int SLAB = 192;
    __shared__ uint2 pool_all[4][POOL_ALLOC];
    __shared__ int segs_all[4][K + 1];
    __shared__ float4 slab_all[4][SLAB + 64];      // + one dummy slot per lane (unconditional writes)
    __shared__ int2 runs_all[4][16];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    uint2* pool = pool_all[wave];
    int* segs = segs_all[wave];
    float4* slab = slab_all[wave];
    int2* runs = runs_all[wave];
    const int j = lane % G;
    const int slot = lane / G;
    const float inv_extent = 1.0f / g.extent;

    float kpr[MODE == 0 ? 3 * K : 1];
    // a pair farther apart than the reach of every kernel point (max |kp| + extent) carries no influence: it is no
    // candidate, and an untruncated row (sorted by distance) is left at the first entry beyond it -- see CUT, kpconv_fwd.hip
    float cut2 = 3.4e38f;
    if (MODE == 0) {
#pragma unroll
        for (int t = 0; t < 3 * K; ++t) kpr[t] = kernel_points[t];
        float rr = 0.0f;
#pragma unroll
        for (int k = 0; k < K; ++k) rr = fmaxf(rr, (kpr[3 * k] * kpr[3 * k] + kpr[3 * k + 1] * kpr[3 * k + 1]) + kpr[3 * k + 2] * kpr[3 * k + 2]);
        const float R = (__builtin_sqrtf(rr) + g.extent) * 1.0001f;
        cut2 = R * R;
    } else if (MODE == 2 && g.rmax) {
        const float R = (g.rmax[0] + g.extent) * 1.0001f;
        cut2 = R * R;
    }

    int64_t item0, istep, iend;
    ws_wave_items(ns, order ? g.ilv : 0, wave, item0, istep, iend);
    CloudGrid gr = grids[0];
    for (int64_t item = item0; item < iend; item += istep) {
        const int64_t s = order ? (int64_t)order[item] : item;
        if (s < gr.s_base || s >= gr.s_base + gr.s_len) {
            int b = 0;
            while (b + 1 < nb && s >= grids[b].s_base + grids[b].s_len) ++b;
            gr = grids[b];
        }
        const float sx = s_pts[3 * s + 0], sy = s_pts[3 * s + 1], sz = s_pts[3 * s + 2];
        const bool from_row = g.rows != nullptr && key_last[s] == ~0ull;
        for (int cg0 = 0; cg0 < ci; cg0 += NCH * CC) {
            float4 acc[NCH];
            float4 gq[NCH];
            bool chok[NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
                gq[c] = make_float4(1.f, 1.f, 1.f, 1.f);
                const int ch = cg0 + c * CC + 4 * j;
                chok[c] = VEC ? (ch + 3 < ci) : (ch < ci);
                if (g.gate && slot == 0 && ch < ci) {
                    const T* gy = reinterpret_cast<const T*>(g.gate) + s * ci + ch;
                    if (VEC) {
                        if (chok[c]) gq[c] = ld4(gy);
                    } else {
                        if (ch + 0 < ci) gq[c].x = ld1(gy + 0);
                        if (ch + 1 < ci) gq[c].y = ld1(gy + 1);
                        if (ch + 2 < ci) gq[c].z = ld1(gy + 2);
                        if (ch + 3 < ci) gq[c].w = ld1(gy + 3);
                    }
                }
            }
            int cnt = 0;
            // flush the pool into the accumulators of every channel chunk (balanced over the S slots)
            auto flush = [&](int total) {
                wave_lds_order();
                total = min(total, POOL);
                const int per = (total + S - 1) / S;
                const int lo = slot * per;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    if (cg0 + c * CC >= ci) continue;                   // wave-uniform (no `break`: the loop must unroll, or
                                                                        // the accumulators land in scratch memory)
                    const int chl = chok[c] ? cg0 + c * CC + 4 * j : 0;
                    const int hi = chok[c] ? min(lo + per, total) : lo;
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
                            acc[c].x = fmaf(w[u], v[u].x, acc[c].x);
                            acc[c].y = fmaf(w[u], v[u].y, acc[c].y);
                            acc[c].z = fmaf(w[u], v[u].z, acc[c].z);
                            acc[c].w = fmaf(w[u], v[u].w, acc[c].w);
                        }
                    }
                }
                wave_lds_order();
            };
            // membership of candidate c (the query) for this support: inside the radius and not cut off q's row
            auto member = [&](const float4& c, bool active, unsigned long long kl) -> bool {
                const float d2 = ref_d2(c.x, c.y, c.z, make_float4(sx, sy, sz, 0.0f));
                const unsigned long long key = nb_key(d2, (unsigned)s);
                return active && d2 < r2 && d2 <= cut2 && key <= kl;
            };
            // ONE loop hands 64-pair batches to ONE inlined copy of the list / flush phases (a lambda that is called from
            // several places is outlined, and everything it captures -- the accumulators, the kernel points -- then lives in
            // scratch memory: the first form of this kernel ran 8 x slower than the transposed-table kernel for that reason).
            //   from_row   the support's own (untruncated) row holds every point within the radius: nearly every entry is a
            //              pair, the chunks go to the list phase directly.  The chain  row entry -> coordinates / key_last
            //              of chunk i + 1 and the row entries of chunk i + 2 are in flight under the work of chunk i.
            //   walk       the nine cell runs around the support, 128 candidates per step; hits are queued in the slab
            //              (capacity 2 x 64 + a dummy slot per lane) and leave it 64 at a time.
            const int nchunk = from_row ? (g.rows_h + 63) >> 6 : 0;
            auto load_q = [&](int ch) -> int64_t {
                const int col = 64 * ch + lane;
                return (ch < nchunk && col < g.rows_h) ? g.rows[s * g.rows_h + col] : -1;
            };
            auto load_c = [&](int64_t qi, float4& c, unsigned long long& kl) -> bool {
                const bool active = qi >= 0 && qi < ns;
                const int64_t qq = active ? qi : 0;
                c = make_float4(s_pts[3 * qq + 0], s_pts[3 * qq + 1], s_pts[3 * qq + 2], __int_as_float((int)qq));
                kl = key_last[qq];
                return active;
            };
            float4 c0 = make_float4(0.f, 0.f, 0.f, 0.f), c1 = c0;
            unsigned long long kl0 = 0, kl1 = 0;
            bool a0 = false, a1 = false;
            int64_t q1 = -1;
            int ch = 0;
            if (from_row) {
                a0 = load_c(load_q(0), c0, kl0);
                q1 = load_q(1);
            }
            int run = 0, rp = 0, re = 0;                       // walk state: next run, position / end inside the current run
            if (!from_row && gr.s_len > 0) {
                const CellBlock k = grid_cell_block(gr, sx, sy, sz);
                if (lane < 9) {     // grid_cell_run (ws_grid.h) for run `lane`, spelt out: through it the deformable instantiations change
                    const int z = k.cz + lane / 3 - 1, y = k.cy + lane % 3 - 1;
                    const bool ok = k.x0 <= k.x1 && z >= 0 && z < gr.nz && y >= 0 && y < gr.ny;
                    const int row = gr.cell_base + ((ok ? z : 0) * gr.ny + (ok ? y : 0)) * gr.nx;
                    runs[lane] = make_int2(ok ? cell_start[row + k.x0] : 0, ok ? cell_start[row + k.x1 + 1] : 0);
                }
                wave_lds_order();
            } else {
                run = 9;
            }
            for (;;) {
                float4 c;
                bool real;
                if (from_row) {
                    if (ch >= nchunk) break;
                    {   // the row is sorted by distance: past the reach (or at the padding) nothing follows
                        const float d2f = ref_d2(c0.x, c0.y, c0.z, make_float4(sx, sy, sz, 0.0f));
                        const float d2_first = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(d2f)));
                        const int a_first = __builtin_amdgcn_readfirstlane(a0 ? 1 : 0);
                        if (!a_first || d2_first > cut2) break;
                    }
                    if (ch + 1 < nchunk) a1 = load_c(q1, c1, kl1);
                    q1 = load_q(ch + 2);
                    c = c0;
                    real = member(c0, a0, kl0);
                    c0 = c1; kl0 = kl1; a0 = a1; a1 = false;
                    ++ch;
                } else {
                    // fill the queue up to 64 hits (or the end of the walk)
                    while (cnt < 64) {
                        if (rp >= re) {
                            if (run >= 9) break;
                            const int2 rr = runs[run++];
                            rp = __builtin_amdgcn_readfirstlane(rr.x);
                            re = __builtin_amdgcn_readfirstlane(rr.y);
                            continue;
                        }
                        const int pa = rp + lane, pb = rp + 64 + lane;
                        const bool aa = pa < re, ab = pb < re;
                        const float4 ca = sorted[aa ? pa : rp], cb = sorted[ab ? pb : rp];
                        const unsigned long long ka = key_last[__float_as_int(ca.w)], kb = key_last[__float_as_int(cb.w)];
                        const bool ha = member(ca, aa, ka), hb = member(cb, ab, kb);
                        const unsigned long long ma = __ballot(ha), mb = __ballot(hb);
                        const int na = __builtin_popcountll(ma);
                        slab[ha ? cnt + lane_rank(ma) : SLAB + lane] = ca;          // cnt < 64 on entry: both batches fit 192
                        slab[hb ? cnt + na + lane_rank(mb) : SLAB + lane] = cb;
                        cnt += na + __builtin_popcountll(mb);
                        rp += 128;
                    }
                    if (cnt == 0) break;
                    wave_lds_order();
                    const int take_n = min(cnt, 64);
                    real = lane < take_n;
                    c = slab[real ? lane : 0];
                    // the remainder (< 128 entries) moves to the front
                    const int rem = cnt - take_n;
                    const float4 t0 = slab[64 + (lane < rem ? lane : 0)];
                    const float4 t1 = slab[128 + (lane + 64 < rem ? lane : 0)];
                    wave_lds_order();
                    if (lane < rem) slab[lane] = t0;
                    if (lane + 64 < rem) slab[64 + lane] = t1;
                    cnt = rem;
                    wave_lds_order();
                }
                // ---- list + flush of this batch: lane = pair (c = the query's coordinates and index; !real = dead lane)
                const int q = real ? __float_as_int(c.w) : 0;
                const float nx = sx - c.x, ny = sy - c.y, nz = sz - c.z;
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
                } else {
                    const float* lkp = deformed_kp ? deformed_kp + (int64_t)q * (3 * K) : kernel_points;
                    const float* lmod = modulations ? modulations + (int64_t)q * K : nullptr;
                    auto kp = [&](int k, int cidx) { return MODE == 0 ? kpr[MODE == 0 ? 3 * k + cidx : 0] : lkp[3 * k + cidx]; };
                    auto nomin = [&](int, float) {};
                    kp_list<K, MODE == 2 ? 1 : MODE>(nx, ny, nz, real, kp, g, inv_extent, (unsigned)(q * K), 1u, lmod, pool, segs, lane,
                                                     total, maxlen, nomin);
                    if (total <= POOL) {
                        flush(total);
                    } else {
                        for (int sub = 0; sub < 4; ++sub) {
                            total = 0; maxlen = 0;
                            kp_list<K, MODE == 2 ? 1 : MODE>(nx, ny, nz, real && (lane >> 4) == sub, kp, g, inv_extent, (unsigned)(q * K),
                                                             1u, lmod, pool, segs, lane, total, maxlen, nomin);
                            flush(total);
                        }
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                if (cg0 + c * CC >= ci) continue;
#pragma unroll
                for (int o = G; o < 64; o <<= 1) {
                    acc[c].x += __shfl_xor(acc[c].x, o, 64);
                    acc[c].y += __shfl_xor(acc[c].y, o, 64);
                    acc[c].z += __shfl_xor(acc[c].z, o, 64);
                    acc[c].w += __shfl_xor(acc[c].w, o, 64);
                }
                if (slot == 0) {
                    const int ch = cg0 + c * CC + 4 * j;
                    T* dst = dx + s * ci + ch;
                    float4 a = acc[c];
                    if (g.gate) {
                        a.x *= gq[c].x > 0.0f ? 1.0f : g.gate_slope; a.y *= gq[c].y > 0.0f ? 1.0f : g.gate_slope;
                        a.z *= gq[c].z > 0.0f ? 1.0f : g.gate_slope; a.w *= gq[c].w > 0.0f ? 1.0f : g.gate_slope;
                    }
                    if (VEC) {
                        if (chok[c]) st4(dst, a);
                    } else {
                        if (ch + 0 < ci) st1(dst + 0, a.x);
                        if (ch + 1 < ci) st1(dst + 1, a.y);
                        if (ch + 2 < ci) st1(dst + 2, a.z);
                        if (ch + 3 < ci) st1(dst + 3, a.w);
                    }
                }
            }
            wave_lds_order();
        }
    }
}

// max |kernel point| over kp4 [n] float4, the value ws_kpconv_deform_prepare hands out as kp_rmax, bit for bit (the same
// expression without contraction, the same correctly rounded root; a maximum does not depend on the order): what
// ws_kpconv_gather_bwd_x_grid_wide bounds its candidates with when the caller passes no kp_rmax.  rmax_bits is zeroed before.
__global__ __launch_bounds__(256) void kp4_rmax_kernel(const float4* __restrict__ kp4, int64_t n, int* __restrict__ rmax_bits)
{
#pragma clang fp contract(off)
    int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) e = n - 1;                                          // (tail lanes redo the last element: every lane reduces)
    const float4 v = kp4[e];
    float r = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) r = fmaxf(r, __shfl_xor(r, o, 64));
    if ((threadIdx.x & 63) == 0 && __float_as_int(r) > *(volatile int*)rmax_bits) atomicMax(rmax_bits, __float_as_int(r));
}

}  // namespace

namespace kpconv {

// kpconv_gather_bwd_x_gridw_kernel for ws_kpconv_gather_bwd_x_grid_wide: MODE 0 or 2; several channel chunks only with G = 16
void launch_bwd_x_gridw(const GatherPlan& p, void* stream, const float* s_pts, int64_t ns, const GridView& v, int32_t nb, const void* dwf,
                        int32_t ci, const float* kernel_points, const GeomParams& g, void* dx, const int32_t* order)
{
    dispatch([&](auto bf, auto gr, auto mode, auto vec, auto nch, auto kn) {
        using T = Row<bf.value>;
        if constexpr ((!bf.value || vec.value) && (nch.value == 1 || gr.value == 16) && (kn.value == 15 || (!bf.value && mode.value == 0)))
            kpconv_gather_bwd_x_gridw_kernel<kn.value, gr.value, mode.value, vec.value != 0, nch.value, T>
                <<<p.grid, 256, 0, (hipStream_t)stream>>>(
                s_pts, ns, v.grids, nb, v.cell_start, v.sorted, v.key_last, v.r2, (const T*)dwf, ci, kernel_points, nullptr, nullptr, g, (T*)dx,
                order);
    }, Flag{p.bf16}, Pick<1, 2, 4, 8, 16>{p.n}, Pick<0, 2>{p.mode}, Flag{p.vec}, Pick<1, 2, 4>{p.nch}, Pick<WS_KP_SIZES>{p.k});
}

void launch_kp4_rmax(void* stream, const float* kp4, int64_t n, float* rmax)
{
    kp4_rmax_kernel<<<(unsigned)ws_ceil_div(n, 256), 256, 0, (hipStream_t)stream>>>(reinterpret_cast<const float4*>(kp4), n,
                                                                                    reinterpret_cast<int*>(rmax));
}

}  // namespace kpconv
