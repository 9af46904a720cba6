// weasal_amd/csrc/kpconv_bwd_geom.hip -- KPConv geometry backward for gfx950 (wave64) and its launches.
//
// K6  kpconv_gather_bwd_geom : d deformed_kp, d modulations (deformable only)
// The VALU form for every influence / aggregation (kpconv_gather_bwd_geom_kernel) and the matrix-core form of the deformable
// fast path with packed kernel points (kpconv_gather_bwd_geom_def_kernel).
#include "kpconv_launch.h"
#include "ws_dispatch.h"

namespace {

// ---------------------------------------------------------------------------------------------
// K6 geometry backward (deformable): gradients of deformed_kp and modulations.
//   dL/dw(q,h,k)   = mod[q,k] * sum_c dwf[q,k,c] * x[idx,c]
//   dL/dmod[q,k]   = sum_h w(q,h,k) * sum_c dwf[q,k,c] * x[idx,c]
//   linear:  dw/dkp = (n - kp) / (extent * sqrt(d2))   where 0 < w
//   gaussian: dw/dkp = w * (n - kp) / (sigma^2 + 0.5e-9)
//   min_d2:  d min_d2[q,k]/dkp = 2 (kp - n_h*) at the arg-min column h*
// One wave per query; lane = neighbour column for the geometry, channels are looped with a wave
// reduction of the per-(h,k) dot products through LDS-staged dwf rows.
// ---------------------------------------------------------------------------------------------
template <int K, typename T = float>
__global__ __launch_bounds__(256) void kpconv_gather_bwd_geom_kernel(
    const float* __restrict__ q_pts, int64_t nq, const float* __restrict__ s_pts, int64_t ns,
    const int64_t* __restrict__ inds, int h, const T* __restrict__ x, int ci,
    const T* __restrict__ dwf, const float* __restrict__ deformed_kp,
    const float* __restrict__ modulations, const float* __restrict__ d_min_d2, GeomParams g,
    float* __restrict__ d_kp, float* __restrict__ d_mod, int vec4)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    for (int64_t q = (int64_t)blockIdx.x * 4 + wave; q < nq; q += (int64_t)gridDim.x * 4) {
        const float qx = q_pts[3 * q + 0], qy = q_pts[3 * q + 1], qz = q_pts[3 * q + 2];
        const float* kp = deformed_kp + q * (3 * K);
        float gk[K][3];
        float gm[K];
        float best[K];      // running (min d2, column) for the min_d2 path
        int bestcol[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            gk[k][0] = gk[k][1] = gk[k][2] = 0.0f;
            gm[k] = 0.0f;
            best[k] = 3.4e38f;
            bestcol[k] = 0x7fffffff;
        }
        for (int h0 = 0; h0 < h; h0 += 64) {
            const int col = h0 + lane;
            const bool incol = col < h;
            int64_t idx = incol ? inds[q * h + col] : ns;
            const bool real = incol && idx < ns && idx >= 0;
            float px = WS_SHADOW, py = WS_SHADOW, pz = WS_SHADOW;
            if (real) { px = s_pts[3 * idx]; py = s_pts[3 * idx + 1]; pz = s_pts[3 * idx + 2]; }
            const float nx = px - qx, ny = py - qy, nz = pz - qz;
            float w[K], d2[K];
            kp_influence<K>(nx, ny, nz, kp, g, real, w, d2);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                // dot[k] = sum_c dwf[q,k,c] * x[idx,c]  (only where the weight is live)
                float dot = 0.0f;
                if (w[k] != 0.0f) {
                    const T* a = dwf + (q * K + k) * ci;
                    const T* b = x + idx * ci;
                    if (vec4) {
                        // 16-byte pieces, four independent partial sums (the per-lane rows are L2 resident)
                        float4 s4 = make_float4(0.f, 0.f, 0.f, 0.f);
                        for (int cc = 0; cc < ci; cc += 4) {
                            const float4 av = ld4(a + cc);
                            const float4 bv = ld4(b + cc);
                            s4.x = fmaf(av.x, bv.x, s4.x); s4.y = fmaf(av.y, bv.y, s4.y);
                            s4.z = fmaf(av.z, bv.z, s4.z); s4.w = fmaf(av.w, bv.w, s4.w);
                        }
                        dot = (s4.x + s4.y) + (s4.z + s4.w);
                    } else {
                        for (int cc = 0; cc < ci; ++cc) dot = fmaf(ld1(a + cc), ld1(b + cc), dot);
                    }
                }
                const float mod = modulations ? modulations[q * K + k] : 1.0f;
                gm[k] += w[k] * dot;
                float coef = 0.0f;   // dL/dw * dw/d(d2) * 2, applied to (kp - n)
                if (w[k] != 0.0f) {
                    const float gw = dot * mod;
                    if (g.influence == WS_INFLUENCE_LINEAR) {
                        const float sd = sqrtf(d2[k]);
                        // w = 1 - sd/ext ; dw/dkp = -(kp - n) / (ext * sd)
                        coef = (sd > 0.0f) ? -gw / (g.extent * sd) : 0.0f;
                    } else if (g.influence == WS_INFLUENCE_GAUSSIAN) {
                        const float sig = g.extent * 0.3f;
                        // w = exp(-d2 / den) ; dw/dkp = -w * 2 (kp - n) / den
                        coef = -gw * w[k] * 2.0f / (2.0f * sig * sig + 1e-9f);
                    }
                }
                gk[k][0] += coef * (kp[3 * k + 0] - nx);
                gk[k][1] += coef * (kp[3 * k + 1] - ny);
                gk[k][2] += coef * (kp[3 * k + 2] - nz);
                if (incol && (d2[k] < best[k])) { best[k] = d2[k]; bestcol[k] = col; }
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            // min_d2 path: wave arg-min (first column wins ties, like torch.min on CPU)
            float gx = ws_wave_sum(gk[k][0]);
            float gy = ws_wave_sum(gk[k][1]);
            float gz = ws_wave_sum(gk[k][2]);
            const float gmod = ws_wave_sum(gm[k]);
            if (d_min_d2) {
                float b = best[k];
                int bc = bestcol[k];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const float ob = __shfl_xor(b, o, 64);
                    const int oc = __shfl_xor(bc, o, 64);
                    if (ob < b || (ob == b && oc < bc)) { b = ob; bc = oc; }
                }
                // the winning lane recomputes its offset
                const int64_t idx = inds[q * h + bc];
                float px = WS_SHADOW, py = WS_SHADOW, pz = WS_SHADOW;
                if (idx < ns && idx >= 0) { px = s_pts[3 * idx]; py = s_pts[3 * idx + 1]; pz = s_pts[3 * idx + 2]; }
                const float gmin = d_min_d2[q * K + k];
                gx += gmin * 2.0f * (kp[3 * k + 0] - (px - qx));
                gy += gmin * 2.0f * (kp[3 * k + 1] - (py - qy));
                gz += gmin * 2.0f * (kp[3 * k + 2] - (pz - qz));
            }
            if (lane == 0) {
                d_kp[(q * K + k) * 3 + 0] = gx;
                d_kp[(q * K + k) * 3 + 1] = gy;
                d_kp[(q * K + k) * 3 + 2] = gz;
                if (d_mod) d_mod[q * K + k] = gmod;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// K6 on the matrix core (deformable fast path: linear influence, sum aggregation, packed kernel points).
// What the geometry backward needs per (query, neighbour h, kernel point k) is the scalar
//     dot[k][h] = sum_c dwf[q,k,c] * x[inds[q,h], c]
// -- per query a dense product  dWF_q (15 x Ci) . X_q^T (Ci x H).  The VALU form above evaluates it only where the
// influence is live, one serial Ci-long chain per lane over two scattered rows (24 ms per config-5 level-0 launch).
// Here it runs as v_mfma_f32_16x16x4_f32 over blocks of 16 neighbours:
//   A  lane (i = lane&15, kk = lane>>4): CK = Ci/4 consecutive channels kk*CK .. of dwf[q, i, :], in registers for the
//      whole query (Ci <= 128; wider rows re-load A per block: those levels hold a few hundred points);
//   B  lane (j = lane&15, kk): the same channels of x[inds[q, 16 b + j], :]  (16 .. 64 contiguous bytes per lane);
//   D  lane (j, g = lane>>4) ends with dot[4g + r][16 b + j], r = 0..3 -- exactly the (neighbour, kernel point) pairs
//      whose geometry that lane then evaluates: influence, d influence / d kernel point, running arg-min of d2.
// Per query: reduce the 4 x (3 + 1) sums over the 16 lanes of a group, add the min_d2 path at the arg-min column,
// one float4 store (d x, d y, d z, d modulation) per kernel point.  Sums are per-lane partial sums combined by a fixed
// shuffle tree: deterministic.
// ---------------------------------------------------------------------------------------------
template <int CK, bool AREG, typename T, bool CUT = false>
__global__ __launch_bounds__(256) void kpconv_gather_bwd_geom_def_kernel(
    const float* __restrict__ q_pts, int64_t nq, const float* __restrict__ s_pts, int64_t ns,
    const int64_t* __restrict__ inds, int h, const T* __restrict__ x, int ci, const T* __restrict__ dwf,
    const float4* __restrict__ kp4, const float* __restrict__ d_min_d2, float extent, float4* __restrict__ d_kp4,
    const int32_t* __restrict__ order)
{
    constexpr int K = 15;
    constexpr int CB = 4 * CK;                                   // channels per pass of the product
    __shared__ float4 nb_all[4][64];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int j = lane & 15, g = lane >> 4;                       // (= i, kk of the A / B operands)
    float4* nb = nb_all[wave];
    const float inv_extent = 1.0f / extent;
    int64_t item0, istep, iend;
    ws_wave_items(nq, 0, wave, item0, istep, iend);
    for (int64_t item = item0; item < iend; item += istep) {
        const int64_t q = order ? (int64_t)order[item] : item;
        float4 kq[4];
        float cm[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = 4 * g + r;
            kq[r] = k < K ? kp4[q * K + k] : make_float4(1.0e9f, 1.0e9f, 1.0e9f, 0.0f);
            cm[r] = kq[r].w * inv_extent;
        }
        const float qx = q_pts[3 * q + 0], qy = q_pts[3 * q + 1], qz = q_pts[3 * q + 2];
        float a[CK];
        auto load_a = [&](int cb) {
            RowLoad<CK, T>::ld(dwf + (q * K + (j < K ? j : 0)) * ci + cb + g * CK, a);
            if (j >= K) {
#pragma unroll
                for (int t = 0; t < CK; ++t) a[t] = 0.0f;
            }
        };
        if (AREG) load_a(0);
        float gk[4][3], gm[4], best[4];
        int bestcol[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            gk[r][0] = gk[r][1] = gk[r][2] = 0.0f;
            gm[r] = 0.0f;
            best[r] = 3.4e38f;
            bestcol[r] = 0x7fffffff;
        }
        // index / coordinates of the first 64 columns
        auto fetch = [&](int h0, int& idx, float& px, float& py, float& pz) {
            const int col = h0 + lane;
            idx = -1;
            if (col < h) { const int64_t v = inds[q * h + col]; idx = (v >= 0 && v < ns) ? (int)v : -1; }
            px = py = pz = WS_SHADOW;
            if (idx >= 0) { px = s_pts[3 * (int64_t)idx]; py = s_pts[3 * (int64_t)idx + 1]; pz = s_pts[3 * (int64_t)idx + 2]; }
        };
        int idx; float px, py, pz;
        fetch(0, idx, px, py, pz);
        float cut2 = 3.4e38f;                                     // CUT: see kpconv_gather_fwd_mfma_kernel (sorted rows)
        for (int h0 = 0; h0 < h; h0 += 64) {
            wave_lds_order();                                     // the previous chunk's readers are done
            int ncut = 64;
            {
                const bool incol = h0 + lane < h;                 // past the row: far beyond the shadow point (never the minimum)
                const float ox = px - qx, oy = py - qy, oz = pz - qz;
                nb[lane] = make_float4(incol ? ox : 3.0e18f, incol ? oy : 3.0e18f, incol ? oz : 3.0e18f, __int_as_float(idx));
                if constexpr (CUT) {
                    const float dn2 = (incol && idx >= 0) ? (ox * ox + oy * oy) + oz * oz : 3.4e38f;
                    ncut = __builtin_popcountll(__ballot(dn2 <= cut2));
                    if (ncut == 0 && h0 > 0) break;
                }
            }
            wave_lds_order();
            if (h0 + 64 < h && ncut == 64) fetch(h0 + 64, idx, px, py, pz);     // next chunk's chain under this chunk's work
            const int nblk = min(4, (min(h - h0, ncut) + 15) >> 4);
            float bv[2][CK];
            float4 nv[2];
            auto load_b = [&](int b4, int slot) {
                nv[slot] = nb[16 * b4 + j];
                if (AREG) {
                    const int nidx = __float_as_int(nv[slot].w);
                    RowLoad<CK, T>::ld(x + (size_t)((unsigned)(nidx >= 0 ? nidx : 0) * (unsigned)ci) + g * CK, bv[slot]);
                }
            };
            auto compute = [&](int b4, int slot) {
                f32x4v acc = f32x4v{0.f, 0.f, 0.f, 0.f};
                const float4 n = nv[slot];
                if (AREG) {
#pragma unroll
                    for (int t = 0; t < CK; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], bv[slot][t], acc, 0, 0, 0);
                } else {
                    const int nidx = __float_as_int(n.w);
                    const T* xr = x + (size_t)((unsigned)(nidx >= 0 ? nidx : 0) * (unsigned)ci) + g * CK;
                    for (int cb = 0; cb < ci; cb += CB) {
                        load_a(cb);
                        float bb[CK];
                        RowLoad<CK, T>::ld(xr + cb, bb);
#pragma unroll
                        for (int t = 0; t < CK; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], bb[t], acc, 0, 0, 0);
                    }
                }
                const int col = h0 + 16 * b4 + j;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float dx = n.x - kq[r].x, dy = n.y - kq[r].y, dz = n.z - kq[r].z;
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    const float rs = __builtin_amdgcn_rsqf(d2);
                    const bool nz = d2 > 0.0f;
                    const float sd = nz ? d2 * rs : 0.0f;
                    const float t = 1.0f - sd * inv_extent;
                    const float w = fmaxf(t, 0.0f);
                    const float dot = acc[r];
                    gm[r] = fmaf(w, dot, gm[r]);
                    // w = 1 - |n - kp| / extent  ->  d w / d kp = (n - kp) / (extent |n - kp|), where 0 < w
                    const float coef = (t > 0.0f && nz) ? dot * cm[r] * rs : 0.0f;
                    gk[r][0] = fmaf(coef, dx, gk[r][0]);
                    gk[r][1] = fmaf(coef, dy, gk[r][1]);
                    gk[r][2] = fmaf(coef, dz, gk[r][2]);
                    const bool lower = d2 < best[r];               // columns ascend per lane: the first minimum stays
                    best[r] = lower ? d2 : best[r];
                    bestcol[r] = lower ? col : bestcol[r];
                }
            };
            load_b(0, 0);
#pragma unroll
            for (int b4 = 0; b4 < 4; ++b4) {
                if (b4 < nblk) {
                    if (b4 + 1 < nblk) load_b(b4 + 1, (b4 + 1) & 1);
                    compute(b4, b4 & 1);
                }
            }
            if constexpr (CUT) {
                if (ncut < 64) break;                             // the row left the cutoff inside this chunk
                if (h0 == 0) {
                    // influence reach and what could still lower a minimum, over this query's 15 kernel points
                    float reach = 0.0f, rq = 0.0f;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float bm = best[r];
#pragma unroll
                        for (int o = 1; o < 16; o <<= 1) bm = fminf(bm, __shfl_xor(bm, o, 64));
                        if (4 * g + r < K) {
                            const float rk = __builtin_sqrtf((kq[r].x * kq[r].x + kq[r].y * kq[r].y) + kq[r].z * kq[r].z);
                            rq = fmaxf(rq, rk);
                            reach = fmaxf(reach, __builtin_sqrtf(bm) + rk);
                        }
                    }
                    float R = fmaxf(rq + extent, reach);
                    R = fmaxf(R, __shfl_xor(R, 16, 64));
                    R = fmaxf(R, __shfl_xor(R, 32, 64));
                    R *= 1.0001f;
                    cut2 = R * R;
                }
            }
        }
        // ---- per kernel point: sums over the 16 lanes of the group, arg-min of d2 (first column wins ties)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                gk[r][0] += __shfl_xor(gk[r][0], o, 64);
                gk[r][1] += __shfl_xor(gk[r][1], o, 64);
                gk[r][2] += __shfl_xor(gk[r][2], o, 64);
                gm[r] += __shfl_xor(gm[r], o, 64);
                const float ob = __shfl_xor(best[r], o, 64);
                const int oc = __shfl_xor(bestcol[r], o, 64);
                const bool take = ob < best[r] || (ob == best[r] && oc < bestcol[r]);
                best[r] = take ? ob : best[r];
                bestcol[r] = take ? oc : bestcol[r];
            }
            const int k = 4 * g + r;
            if (k < K) {
                float gx = gk[r][0], gy = gk[r][1], gz = gk[r][2];
                if (d_min_d2) {
                    // d min_d2[q,k] / d kp = 2 (kp - n) at the arg-min column (shadow columns take part, blocks.py:278-304)
                    const int64_t v = inds[q * h + min(bestcol[r], h - 1)];
                    float mx = WS_SHADOW, my = WS_SHADOW, mz = WS_SHADOW;
                    if (v >= 0 && v < ns) { mx = s_pts[3 * v]; my = s_pts[3 * v + 1]; mz = s_pts[3 * v + 2]; }
                    const float gmin = 2.0f * d_min_d2[q * K + k];
                    gx = fmaf(gmin, kq[r].x - (mx - qx), gx);
                    gy = fmaf(gmin, kq[r].y - (my - qy), gy);
                    gz = fmaf(gmin, kq[r].z - (mz - qz), gz);
                }
                if (j == 0) d_kp4[q * K + k] = make_float4(gx, gy, gz, gm[r]);
            }
        }
    }
}

}  // namespace

namespace kpconv {

// kpconv_gather_bwd_geom_kernel for ws_kpconv_gather_bwd_geom / _bf16; whether the rows move as float4 pieces is an argument (p.vec)
void launch_bwd_geom(const GatherPlan& p, void* stream, const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int64_t* inds,
                     int32_t h, const void* x, int32_t ci, const void* dwf, const float* deformed_kp, const float* modulations,
                     const float* d_min_d2, const GeomParams& g, float* d_deformed_kp, float* d_modulations)
{
    dispatch([&](auto bf, auto kn) {
        using T = Row<bf.value>;
        if constexpr (kn.value == 15 || !bf.value)
            kpconv_gather_bwd_geom_kernel<kn.value, T><<<p.grid, 256, 0, (hipStream_t)stream>>>(
                q_pts, nq, s_pts, ns, inds, h, (const T*)x, ci, (const T*)dwf, deformed_kp, modulations, d_min_d2, g, d_deformed_kp,
                d_modulations, p.vec);
    }, Flag{p.bf16}, Pick<WS_KP_SIZES>{p.k});
}

// kpconv_gather_bwd_geom_def_kernel for ws_kpconv_gather_bwd_geom_def
void launch_bwd_geom_def(const GatherPlan& p, void* stream, const float* q_pts, int64_t nq, const float* s_pts, int64_t ns,
                         const int64_t* inds, int32_t h, const void* x, int32_t ci, const void* dwf, const float* kp4, const float* d_min_d2,
                         float extent, float* d_kp4, const int32_t* order)
{
    dispatch([&](auto bf, auto ck, auto areg, auto cut) {
        using T = Row<bf.value>;
        kpconv_gather_bwd_geom_def_kernel<ck.value, areg.value != 0, T, cut.value != 0><<<p.grid, 256, 0, (hipStream_t)stream>>>(
            q_pts, nq, s_pts, ns, inds, h, (const T*)x, ci, (const T*)dwf, reinterpret_cast<const float4*>(kp4), d_min_d2, extent,
            reinterpret_cast<float4*>(d_kp4), order);
    }, Flag{p.bf16}, Pick<4, 8, 16, 32>{p.n}, Flag{p.areg}, Flag{p.cut});
}

}  // namespace kpconv
