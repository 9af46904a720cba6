// weasal_amd/csrc/kpconv_device.h -- what the KPConv gather kernel families share on the device (gfx950, wave64).
//
// Reference semantics: models/blocks.py:238-374 (KPConv.forward) and its autograd.  The families, one unit each:
//   K3   kpconv_fwd.hip        forward gather           K4G  kpconv_bwd_grid.hip, kpconv_bwd_gridw.hip  K4 without a transposed table
//   K4   kpconv_bwd_x.hip      backward w.r.t. x        K6   kpconv_bwd_geom.hip                        geometry backward (deformable)
// Here: the launch parameters every kernel takes (GeomParams), the influence of the kernel points, and the list phase of
// the entry pool that K3, K4 and K4G run (its structure is described above the pool constants).  kpconv.hip holds the
// entries and every selection rule; kpconv_launch.h is what crosses from there into the family units.
#pragma once
#include "ws_common.h"
#include "ws_grid.h"
#include "ws_bf16.h"

namespace kpconv {

struct GeomParams {
    float extent;
    int influence;
    int aggregation;
    int deformable;   // 1: apply the in-range filter of blocks.py:301-325
    const void* gate; // K4 / K4G only: rows [ns, ci] of the activated output y of the layer that produced x; the stored
    float gate_slope; // gradient is dx * LeakyReLU'(y) (1 where y > 0, gate_slope elsewhere) -- the activation backward
                      // of the preceding unary block folded into the store.  NULL: plain dx.
    const int64_t* rows;  // K4G only: the index matrix [ns, rows_h] of the SAME self-query search the grid belongs to (NULL:
    int rows_h;           // none).  A support whose own row was not truncated (key_last[s] = "infinity") holds every
                          // point within the radius in that row -- a superset of the queries that kept s -- so its
                          // candidates are the row's entries instead of the 27-cell walk.
    const float4* kp4;    // MODE 2 only (deformable / modulated, linear influence, sum): the per-query kernel points packed as
                          // [nq, 15] float4 = (x, y, z, modulation) -- ONE aligned 16-byte load per (query, kernel point)
                          // where the reference-shaped operands deformed_kp [nq,15,3] + modulations [nq,15] need four.
    const float* rmax;    // K4G, MODE 2: device float = max over the queries of (max_k |kp_k|), written by
                          // ws_kpconv_deform_prepare: a pair farther apart than that + extent has no influence (NULL: no bound)
    int cut;              // pool-form K3 (MODE 0): 1 = rows are sorted by distance, stop at the influence reach (see CUT)
    int ilv;              // K4G: workgroups per XCD of the interleaved item assignment (ws_wave_items), 0 = contiguous chunks
    int csplit;           // matrix-core K3 (rigid): > 1 = an item is (query, one of csplit runs of channel blocks) instead of a query
                          // with all its blocks one after the other -- few queries with wide rows (the deep levels: 275 x 512)
                          // otherwise leave most SIMDs without a wave; the influences are recomputed per block either way
};

// the contraction operands of the fused forward layer (kpconv_fwd.hip: FUSE)
struct FuseArgs {
    const float* w;        // [15 * ci, co] row-major (the module's weights [15, ci, co])
    const float* bias;     // [co] or NULL
    float slope;           // LeakyReLU slope (act != 0)
    int act;
    float* out;            // [nq, co]
};

}  // namespace kpconv
// (named, because these types are in the signatures of the launch_* functions that cross units; the kernels and the helpers
// below stay in each unit's unnamed namespace and name them unqualified)
using namespace kpconv;

namespace {

constexpr float WS_SHADOW = 1e6f;

// Influence of the K kernel points on one neighbour offset n = s - q.  kp is wave-uniform.
// Returns w[K] (0 where no influence) and d2[K].
template <int K>
__device__ __forceinline__ void kp_influence(float nx, float ny, float nz, const float* __restrict__ kp,
                                             const GeomParams& g, bool live, float (&w)[K], float (&d2)[K])
{
    float best = 3.4e38f;
    int arg = 0;
    bool inrange = false;
    const float e2 = g.extent * g.extent;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float dx = nx - kp[3 * k + 0];
        const float dy = ny - kp[3 * k + 1];
        const float dz = nz - kp[3 * k + 2];
        const float d = (dx * dx + dy * dy) + dz * dz;
        d2[k] = d;
        if (d < best) { best = d; arg = k; }
        inrange |= d < e2;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float v;
        if (g.influence == WS_INFLUENCE_LINEAR) {
            v = fmaxf(1.0f - sqrtf(d2[k]) / g.extent, 0.0f);
        } else if (g.influence == WS_INFLUENCE_CONSTANT) {
            v = 1.0f;
        } else {
            const float sig = g.extent * 0.3f;
            v = expf(-d2[k] / (2.0f * sig * sig + 1e-9f));
        }
        if (g.aggregation == WS_AGGREGATION_CLOSEST && k != arg) v = 0.0f;
        if (!live || (g.deformable && !inrange)) v = 0.0f;
        w[k] = v;
    }
}

// LDS-only ordering inside one wave: the wavefront-scope release/acquire fences of wave_lds_sync (ws_grid.h) make the compiler drain EVERY
// outstanding vector-memory load (s_waitcnt vmcnt(0)), i.e. they expose the full latency of loads that were issued on
// purpose ahead of their use.  A wave's own LDS writes and reads are ordered by the LDS queue; what is needed is that the
// compiler keeps them in program order and that the wave's earlier LDS operations have completed.
__device__ __forceinline__ void wave_lds_order()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// ---------------------------------------------------------------------------------------------
// Pool + accumulate structure shared by K3 (forward) and K4 (backward w.r.t. x).
//
// One wave owns one query (K3) / one support (K4) at a time and alternates two phases:
//   list phase   lane = neighbour column (K3) or incoming pair (K4).  The influence of each kernel
//                point is evaluated in registers and the non-zero ones are compacted (v_cmp mask +
//                mbcnt rank) into the wave's LDS entry pool as (row, weight), kernel point after
//                kernel point, so the pool is grouped by kernel point (segs[k] = start of k).
//                With `linear` influence ~1 of the 15 kernel points is non-zero per neighbour: the
//                pool holds ~H entries instead of 15*H.
//   flush phase  lane = (entry slot, 16-byte piece of the row): G lanes read one feature-row
//                segment as float4 straight from L2/HBM (a row is 4*ci contiguous bytes -> 64..256
//                byte coalesced segments, no staging copy), S = 64/G entries per step, register
//                accumulation, no atomics (LDS float atomics were measured at ~1 lane/clk on gfx950).
//
// What bounds these kernels is the scalar unit (one SALU per CU) and divergent-branch bookkeeping,
// not HBM: profiles/r01 showed ~520 SALU instructions per query.  Hence
//   * MODE 0 (rigid kernel, linear influence, sum aggregation -- every shipped configuration) is a
//     separate instantiation: no per-kernel-point mode dispatch, the 15 kernel points live in SGPRs
//     for the whole launch, the list phase is fully unrolled;
//   * pool writes are unconditional (lanes without an entry write to a private dummy slot) and the
//     flush loops are branch free (lanes past the end of their segment carry weight 0 and read
//     row 0), so no exec-mask save/restore sits in any inner loop;
//   * pool overflow (only possible with dense influence modes or collapsed deformed kernels) is
//     handled after the fact: the chunk is redone in four 16-lane sub-chunks that always fit.
// MODE 1 keeps every influence / aggregation / deformable combination behind runtime switches.
// ---------------------------------------------------------------------------------------------
constexpr int POOL = 256;                 // real entries per wave (8 B each), >= 16 * 15
constexpr int POOL_ALLOC = POOL + 8 + 128; // + read-past slack of the flush + two dummy slots per lane

// influence of ONE kernel point (same formulas as kp_influence)
__device__ __forceinline__ float kp_weight(float d2, const GeomParams& g, float inv_extent)
{
    if (g.influence == WS_INFLUENCE_LINEAR) return fmaxf(1.0f - __builtin_amdgcn_sqrtf(d2) * inv_extent, 0.0f);
    if (g.influence == WS_INFLUENCE_CONSTANT) return 1.0f;
    const float sig = g.extent * 0.3f;
    return __expf(-d2 / (2.0f * sig * sig + 1e-9f));
}

// 16-byte piece of a feature row, branch free.  VEC: the caller guarantees ch+3 < ci (or passes
// ch = 0 together with a zero weight).  !VEC: element-wise with clamped columns; columns >= ci
// are zeroed.
template <bool VEC, typename T>
__device__ __forceinline__ float4 load_row_piece(const T* __restrict__ base, unsigned row, int ci, int ch)
{
    // 32-bit element offset (the launcher checks rows * ci < 2^31): one v_mul_lo_u32 + one 64-bit add
    const T* src = base + (size_t)(row * (unsigned)ci);
    if (VEC) return ld4(src + ch);          // 16 bytes of f32 / 8 bytes of bf16 (ws_bf16.h)
    float4 v;
    const int last = ci - 1;
    v.x = ld1(src + min(ch + 0, last)); v.y = ld1(src + min(ch + 1, last)); v.z = ld1(src + min(ch + 2, last)); v.w = ld1(src + min(ch + 3, last));
    if (ch + 0 >= ci) v.x = 0.f;
    if (ch + 1 >= ci) v.y = 0.f;
    if (ch + 2 >= ci) v.z = 0.f;
    if (ch + 3 >= ci) v.w = 0.f;
    return v;
}

// keeps a pool read unconditional: without it the compiler sinks `ok ? pool[i] : 0` back under an
// exec-mask branch (s_and_saveexec + s_cbranch per entry -- the scalar unit is the bottleneck here)
__device__ __forceinline__ void keep_unconditional(uint2& e) { asm volatile("" : "+v"(e.x), "+v"(e.y)); }

// Squared distance and influence of the list phase.  Which of the products of (dx dx + dy dy) + dz dz the compiler fuses is its
// choice per instantiation, and K4G summed in index order has to give the bits of K4 (kpconv_bwd_grid_kernels.h): two kernels
// that round a weight differently do not.  K = 15 keeps the plain expressions, whose contraction is part of the code it has
// always had (and agrees between its families); the other sizes spell the fused form out, one rounding sequence everywhere.
template <int K>
__device__ __forceinline__ float list_d2(float dx, float dy, float dz)
{
    if constexpr (K == 15) return (dx * dx + dy * dy) + dz * dz;
    else return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
}
template <int K>
__device__ __forceinline__ float list_linear(float d2, float inv_extent)
{
    if constexpr (K == 15) return fmaxf(1.0f - __builtin_amdgcn_sqrtf(d2) * inv_extent, 0.0f);
    else return fmaxf(__builtin_fmaf(-__builtin_amdgcn_sqrtf(d2), inv_extent, 1.0f), 0.0f);
}
template <int K>
__device__ __forceinline__ float list_weight(float d2, const GeomParams& g, float inv_extent)
{
    if (K != 15 && g.influence == WS_INFLUENCE_LINEAR) return list_linear<K>(d2, inv_extent);
    return kp_weight(d2, g, inv_extent);
}

// List phase for one 64-lane chunk.  KPF: kp(k, c) -> coordinate c of kernel point k (SGPR array,
// wave-uniform pointer or per-lane pointer).  Entry row = row_base + k * row_step.
// MINF: optional per-kernel-point hook (k, d2) used by the deformable forward for min_d2.
template <int K, int MODE, typename KPF, typename MINF>
__device__ __forceinline__ void kp_list(float nx, float ny, float nz, bool live, KPF kp, const GeomParams& g,
                                        float inv_extent, unsigned row_base, unsigned row_step, const float* __restrict__ lane_mod,
                                        uint2* pool, int* segs, int lane, int& total, int& maxlen, MINF minf)
{
    const unsigned dummy = POOL + 8 + lane;
    auto emit = [&](int k, float w) {
        const unsigned long long m = __ballot(w != 0.0f);
        const unsigned pos = (unsigned)(total + lane_rank(m));
        const bool ok = (w != 0.0f) && pos < (unsigned)POOL;
        pool[ok ? pos : dummy] = make_uint2(row_base + (unsigned)k * row_step, __float_as_uint(w));
        segs[k] = total;                                   // every lane, same value
        const int c = __builtin_popcountll(m);
        total += c;
        maxlen = max(maxlen, c);
    };
    if (MODE == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float dx = nx - kp(k, 0), dy = ny - kp(k, 1), dz = nz - kp(k, 2);
            const float d = list_d2<K>(dx, dy, dz);
            float w = list_linear<K>(d, inv_extent);
            w = live ? w : 0.0f;
            emit(k, w);
        }
    } else {
        constexpr int KU = K % 3 == 0 ? 3 : 1;      // kernel points per trip of the rolled loops
        const float e2 = g.extent * g.extent;
        int arg = 0;
        if (g.deformable || g.aggregation == WS_AGGREGATION_CLOSEST) {
            float best = 3.4e38f;
            bool inrange = false;
#pragma unroll 1
            for (int kb = 0; kb < K; kb += KU) {
#pragma unroll
                for (int u = 0; u < KU; ++u) {
                    const int k = kb + u;
                    const float dx = nx - kp(k, 0), dy = ny - kp(k, 1), dz = nz - kp(k, 2);
                    const float d = list_d2<K>(dx, dy, dz);
                    if (d < best) { best = d; arg = k; }
                    inrange |= d < e2;
                }
            }
            if (g.deformable) live = live && inrange;
        }
#pragma unroll 1
        for (int kb = 0; kb < K; kb += KU) {
#pragma unroll
            for (int u = 0; u < KU; ++u) {
                const int k = kb + u;
                const float dx = nx - kp(k, 0), dy = ny - kp(k, 1), dz = nz - kp(k, 2);
                const float d = list_d2<K>(dx, dy, dz);
                minf(k, d);
                float w = list_weight<K>(d, g, inv_extent);
                if (g.aggregation == WS_AGGREGATION_CLOSEST && k != arg) w = 0.0f;
                w = live ? w : 0.0f;
                if (lane_mod && w != 0.0f) w *= lane_mod[k];
                emit(k, w);
            }
        }
    }
    segs[K] = total;
}

// List phase for TWO 64-lane column chunks at once (rigid / linear / sum only): lane = columns c and
// c + 64.  Rows of 65..128 neighbours (the calibrated limits of the deeper pyramid levels sit at
// 70-75) then need ONE pool and ONE flush instead of a second, nearly empty chunk that re-reads and
// re-writes all K rows of wf[q].
template <int K, typename KPF>
__device__ __forceinline__ void kp_list2(float ax, float ay, float az, bool alive, unsigned arow, float bx, float by, float bz,
                                         bool blive, unsigned brow, KPF kp, float inv_extent, uint2* pool, int* segs, int lane,
                                         int& total, int& maxlen)
{
    const unsigned dummy_a = POOL + 8 + lane, dummy_b = POOL + 8 + 64 + lane;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float kx = kp(k, 0), ky = kp(k, 1), kz = kp(k, 2);
        const float dxa = ax - kx, dya = ay - ky, dza = az - kz;
        const float dxb = bx - kx, dyb = by - ky, dzb = bz - kz;
        float wa = fmaxf(1.0f - __builtin_amdgcn_sqrtf((dxa * dxa + dya * dya) + dza * dza) * inv_extent, 0.0f);
        float wb = fmaxf(1.0f - __builtin_amdgcn_sqrtf((dxb * dxb + dyb * dyb) + dzb * dzb) * inv_extent, 0.0f);
        wa = alive ? wa : 0.0f;
        wb = blive ? wb : 0.0f;
        const unsigned long long ma = __ballot(wa != 0.0f), mb = __ballot(wb != 0.0f);
        const int ca = __builtin_popcountll(ma), cb = __builtin_popcountll(mb);
        const unsigned pa = (unsigned)(total + lane_rank(ma)), pb = (unsigned)(total + ca + lane_rank(mb));
        const bool oka = (wa != 0.0f) && pa < (unsigned)POOL, okb = (wb != 0.0f) && pb < (unsigned)POOL;
        pool[oka ? pa : dummy_a] = make_uint2(arow, __float_as_uint(wa));
        pool[okb ? pb : dummy_b] = make_uint2(brow, __float_as_uint(wb));
        segs[k] = total;
        total += ca + cb;
        maxlen = max(maxlen, ca + cb);
    }
    segs[K] = total;
}

// List phase of the deformable fast path (MODE 2: per-query kernel points + modulations, linear influence, sum
// aggregation; models/blocks.py:244-267, 287-291, 330-346, 366-367).  lane = pair; `kq` = the 15 packed kernel points
// (x, y, z, modulation) of the pair's QUERY: 15 independent 16-byte loads, all issued before the first use.  One pass:
// the in-range filter of blocks.py:301-325 is implied by the linear influence (a neighbour with no kernel point inside
// the extent has 15 zero influences), and the modulation multiplies the weight (d wf / d x = mod * w).
template <int K>
__device__ __forceinline__ void kp_list_def(float nx, float ny, float nz, bool live, const float4* __restrict__ kq,
                                            float inv_extent, unsigned row_base, uint2* pool, int* segs, int lane, int& total,
                                            int& maxlen)
{
    const unsigned dummy = POOL + 8 + lane;
    float4 kp[K];
#pragma unroll
    for (int k = 0; k < K; ++k) kp[k] = kq[k];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float dx = nx - kp[k].x, dy = ny - kp[k].y, dz = nz - kp[k].z;
        const float d = (dx * dx + dy * dy) + dz * dz;
        float w = fmaxf(1.0f - __builtin_amdgcn_sqrtf(d) * inv_extent, 0.0f) * kp[k].w;
        w = live ? w : 0.0f;
        const unsigned long long m = __ballot(w != 0.0f);
        const unsigned pos = (unsigned)(total + lane_rank(m));
        const bool ok = (w != 0.0f) && pos < (unsigned)POOL;
        pool[ok ? pos : dummy] = make_uint2(row_base + (unsigned)k, __float_as_uint(w));
        segs[k] = total;
        const int c = __builtin_popcountll(m);
        total += c;
        maxlen = max(maxlen, c);
    }
    segs[K] = total;
}

// ---- the matrix-core kernels (K3 in kpconv_fwd.hip, K6 in kpconv_bwd_geom.hip): the accumulator of v_mfma_f32_16x16x4_f32 and
//      NT consecutive channels of a feature row as one load / store
typedef float f32x4v __attribute__((ext_vector_type(4)));

template <int NT, typename T> struct RowLoad;
template <int NT> struct RowLoad<NT, float> {
    static __device__ __forceinline__ void ld(const float* p, float (&v)[NT])
    {
        if constexpr (NT == 1) v[0] = *p;
        else if constexpr (NT == 2) { const float2 a = *reinterpret_cast<const float2*>(p); v[0] = a.x; v[1] = a.y; }
        else {
#pragma unroll
            for (int t = 0; t < NT; t += 4) {
                const float4 a = *reinterpret_cast<const float4*>(p + t);
                v[t] = a.x; v[t + 1] = a.y; v[t + 2] = a.z; v[t + 3] = a.w;
            }
        }
    }
    static __device__ __forceinline__ void st(float* p, const float (&v)[NT])
    {
        if constexpr (NT == 1) *p = v[0];
        else if constexpr (NT == 2) *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
        else {
#pragma unroll
            for (int t = 0; t < NT; t += 4) *reinterpret_cast<float4*>(p + t) = make_float4(v[t], v[t + 1], v[t + 2], v[t + 3]);
        }
    }
};
template <int NT> struct RowLoad<NT, bf16_t> {
    static __device__ __forceinline__ void ld(const bf16_t* p, float (&v)[NT])
    {
        if constexpr (NT == 1) v[0] = ld1(p);
        else if constexpr (NT == 2) { const unsigned a = *reinterpret_cast<const unsigned*>(p); v[0] = ws_bf_lo(a); v[1] = ws_bf_hi(a); }
        else if constexpr (NT == 4) { const float4 a = ld4(p); v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; }
        else {
#pragma unroll
            for (int t = 0; t < NT; t += 8) {
                const uint4 a = *reinterpret_cast<const uint4*>(p + t);
                v[t] = ws_bf_lo(a.x); v[t + 1] = ws_bf_hi(a.x); v[t + 2] = ws_bf_lo(a.y); v[t + 3] = ws_bf_hi(a.y);
                v[t + 4] = ws_bf_lo(a.z); v[t + 5] = ws_bf_hi(a.z); v[t + 6] = ws_bf_lo(a.w); v[t + 7] = ws_bf_hi(a.w);
            }
        }
    }
    static __device__ __forceinline__ void st(bf16_t* p, const float (&v)[NT])
    {
        if constexpr (NT == 1) st1(p, v[0]);
        else if constexpr (NT == 2) *reinterpret_cast<unsigned*>(p) = ws_pack_bf2(v[0], v[1]);
        else if constexpr (NT == 4) st4(p, make_float4(v[0], v[1], v[2], v[3]));
        else {
#pragma unroll
            for (int t = 0; t < NT; t += 8)
                *reinterpret_cast<uint4*>(p + t) = make_uint4(ws_pack_bf2(v[t], v[t + 1]), ws_pack_bf2(v[t + 2], v[t + 3]),
                                                              ws_pack_bf2(v[t + 4], v[t + 5]), ws_pack_bf2(v[t + 6], v[t + 7]));
        }
    }
};

}  // namespace
