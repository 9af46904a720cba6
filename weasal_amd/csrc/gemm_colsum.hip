// weasal_amd/csrc/gemm_colsum.hip -- act_bwd_colsum_kernel and its launcher: the activation backward fused with the column
// sums of the bias gradient.  The plan (ColsumPlan) is gemm.hip's colsum_plan; the chunk sums are gemm_xty.hip's
// reduce_partials_kernel, launched by the entry through launch_reduce_partials.
#include "gemm_launch.h"

namespace {

// ---------------------------------------------------------------------------------------------
// dz = LeakyReLU'(y) * dy and the column sums of dz (the bias gradient of a BatchNormBlock,
// models/blocks.py:465) in ONE pass over [m, n]: partial column sums per row chunk (threads = column
// groups x row lanes, row lanes added through LDS in a fixed order), chunks added by
// reduce_partials_kernel.  V = 4: float4 columns; V = 1: any n.
// ---------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void act_bwd_colsum_kernel(const float* __restrict__ dy, const float* __restrict__ yact,
                                                              int64_t m, int n, int64_t lddy, int64_t ldy, float slope,
                                                              float* __restrict__ dz, int64_t lddz,
                                                              float* __restrict__ partial, int64_t chunk, const WsDrop drop)
{
    // drop.on: dy is the gradient of a DROPPED tensor (nn.Dropout applied to the activated output y, fused into the producing
    // epilogue): g = keep(row * n + col) ? g * scale : 0 first, exactly the separate dropout backward, then the activation
    __shared__ float red[256 * V];
    const int t = threadIdx.x;
    const int ncg = (n + V - 1) / V;                    // column groups
    const int per = ncg < 256 ? ncg : 256;              // column groups per pass
    const int R = 256 / per;                            // row lanes
    const int rl = t / per, cgl = t % per;
    const int64_t mbeg = (int64_t)blockIdx.x * chunk;
    const int64_t mend = mbeg + chunk < m ? mbeg + chunk : m;
    {   // one pass of `per` column groups per workgroup row of the grid (blockIdx.y)
        const int cg = (int)blockIdx.y * per + cgl;
        const int col = cg * V;
        float s[V];
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = 0.0f;
        if (rl < R && cg < ncg) {
            typedef float vec_t __attribute__((ext_vector_type(V)));
            const int64_t sdy = (int64_t)R * lddy, sy = (int64_t)R * ldy, sdz = (int64_t)R * lddz;
            const float* pg = dy + (mbeg + rl) * lddy + col;
            const float* pa = yact ? yact + (mbeg + rl) * ldy + col : nullptr;
            float* pz = yact ? dz + (mbeg + rl) * lddz + col : nullptr;
            auto one = [&](vec_t g, vec_t a, float* out, int64_t row) {
                if (drop.on) {
                    const unsigned long long i0 = (unsigned long long)(row * n + col);
#pragma unroll
                    for (int e = 0; e < V; ++e) g[e] = ws_drop1(g[e], drop, i0 + e);
                }
                if (pa) {
#pragma unroll
                    for (int e = 0; e < V; ++e) g[e] = a[e] > 0.0f ? g[e] : g[e] * slope;
                    *reinterpret_cast<vec_t*>(out) = g;
                }
#pragma unroll
                for (int e = 0; e < V; ++e) s[e] += g[e];
            };
            int64_t r = mbeg + rl;
            for (; r + 3 * R < mend; r += 4 * R) {        // four independent rows in flight per thread
                vec_t g0 = *reinterpret_cast<const vec_t*>(pg), g1 = *reinterpret_cast<const vec_t*>(pg + sdy);
                vec_t g2 = *reinterpret_cast<const vec_t*>(pg + 2 * sdy), g3 = *reinterpret_cast<const vec_t*>(pg + 3 * sdy);
                vec_t a0 = g0, a1 = g1, a2 = g2, a3 = g3;
                if (pa) {
                    a0 = *reinterpret_cast<const vec_t*>(pa); a1 = *reinterpret_cast<const vec_t*>(pa + sy);
                    a2 = *reinterpret_cast<const vec_t*>(pa + 2 * sy); a3 = *reinterpret_cast<const vec_t*>(pa + 3 * sy);
                }
                one(g0, a0, pz, r); one(g1, a1, pz + sdz, r + R); one(g2, a2, pz + 2 * sdz, r + 2 * R); one(g3, a3, pz + 3 * sdz, r + 3 * R);
                pg += 4 * sdy;
                if (pa) { pa += 4 * sy; pz += 4 * sdz; }
            }
            for (; r < mend; r += R) {
                vec_t g0 = *reinterpret_cast<const vec_t*>(pg);
                vec_t a0 = pa ? *reinterpret_cast<const vec_t*>(pa) : g0;
                one(g0, a0, pz, r);
                pg += sdy;
                if (pa) { pa += sy; pz += sdz; }
            }
        }
        if (partial) {
#pragma unroll
            for (int e = 0; e < V; ++e) red[t * V + e] = s[e];
            __syncthreads();
            if (rl == 0 && cg < ncg) {
                for (int q = 1; q < R; ++q)
#pragma unroll
                    for (int e = 0; e < V; ++e) s[e] += red[(q * per + cgl) * V + e];
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (col + e < n) partial[(int64_t)blockIdx.x * n + col + e] = s[e];
            }
            __syncthreads();
        }
    }
}

}  // namespace

namespace gemm {

int launch_act_bwd_colsum(const ColsumPlan& p, const float* dy, int64_t m, int32_t n, int64_t lddy, const float* y, int64_t ldy,
                          float slope, float* dz, int64_t lddz, const WsDrop& drop, hipStream_t st)
{
    const bool called = dispatch([&](auto v) {
        act_bwd_colsum_kernel<v.value><<<p.grid, 256, 0, st>>>(dy, y, m, n, lddy, ldy, slope, dz, lddz, p.partial, p.chunk, drop);
    }, Pick<1, 4>{p.v});
    return called ? WS_OK : ws_no_instantiation("act_bwd_colsum_kernel<V=%d>", p.v);
}

}  // namespace gemm
