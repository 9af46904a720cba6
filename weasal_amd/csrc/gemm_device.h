// weasal_amd/csrc/gemm_device.h -- what the dense-product family units (gemm_xb.hip, gemm_xty.hip, gemm_colsum.hip) share on
// the device side: the vector types, the epilogue gates (XbGate and what applies it), the guarded float4 load, and the index
// of a grouped launch with the host struct that fills it.  Everything is in the anonymous namespace, as the kernels are: the
// kernels' names carry these types (..._GLOBAL__N_1...XbGate...), and the profiles, bench.py and the reporters spell those names.
// That is also why no launch_* function of gemm_launch.h takes one of them: a function with such a parameter is local to its unit.
#pragma once
#include "gemm_launch.h"

using namespace gemm;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Optional multiplicative gates of the GEMM epilogues (applied after bias / residual / activation):
//   y    rows [m, n] (pitch ld) of ANOTHER layer's activated output: v *= LeakyReLU'(y) = (y > 0 ? 1 : slope) -- the
//        activation backward of the layer that consumes this product as its gradient (dX = dY W^T gated by that layer's y);
//   mask rows [m, n] of bytes (pitch ldm): v = mask ? v * mscale : 0 -- dropout, forward (on the activated output) and
//        backward (on the gradient) alike.
//   drop (drop.on): nn.Dropout with the keep decision recomputed from (seed, row * dn + col) -- dn = the row length of the
//        contiguous tensor the reference's droplayer sees -- instead of read from a mask: v = keep ? v * scale : 0.
struct XbGate {
    const float* y; int64_t ld; float slope;
    const uint8_t* mask; int64_t ldm; float mscale;
    WsDrop drop; int64_t dn;
    // rrows (NULL = none): the residual row of output row r is residual[rrows[r * rld]] instead of residual[r] -- a row gather
    // (closest_pool / nearest upsampling, blocks.py:80-92) read by the epilogue instead of written out first; indices outside
    // [0, rn) are the shadow row: zeros
    const int64_t* rrows; int64_t rld; int64_t rn;
};
// first float of the residual row of output row `row` (NULL: the shadow row, or no residual)
__device__ __forceinline__ const float* xb_res_row(const float* residual, int64_t ldr, const XbGate& g, int64_t row)
{
    if (!residual) return nullptr;
    if (!g.rrows) return residual + row * ldr;
    const int64_t i = g.rrows[row * g.rld];
    return (i >= 0 && i < g.rn) ? residual + i * ldr : nullptr;
}
// order: dropout, then the LeakyReLU' gate, then the byte mask -- as a backward, dropout_bwd then activation_bwd is the order the
// separate passes run in (d u = dropout_bwd(d x_d); dz = d u * lrelu'(u)); as a forward only one of them is set
__device__ __forceinline__ void xb_gate4(float4& v, const XbGate& g, int64_t row, int col)
{
    if (g.drop.on) {
        const unsigned long long i = (unsigned long long)(row * g.dn + col);
        v.x = ws_drop1(v.x, g.drop, i); v.y = ws_drop1(v.y, g.drop, i + 1);
        v.z = ws_drop1(v.z, g.drop, i + 2); v.w = ws_drop1(v.w, g.drop, i + 3);
    }
    if (g.y) {
        const float4 q = *reinterpret_cast<const float4*>(g.y + row * g.ld + col);
        v.x *= q.x > 0.0f ? 1.0f : g.slope; v.y *= q.y > 0.0f ? 1.0f : g.slope;
        v.z *= q.z > 0.0f ? 1.0f : g.slope; v.w *= q.w > 0.0f ? 1.0f : g.slope;
    }
    if (g.mask) {
        const unsigned mk = *reinterpret_cast<const unsigned*>(g.mask + row * g.ldm + col);
        v.x = (mk & 0xffu) ? v.x * g.mscale : 0.0f;       v.y = (mk & 0xff00u) ? v.y * g.mscale : 0.0f;
        v.z = (mk & 0xff0000u) ? v.z * g.mscale : 0.0f;   v.w = (mk & 0xff000000u) ? v.w * g.mscale : 0.0f;
    }
}
__device__ __forceinline__ float xb_gate1(float v, const XbGate& g, int64_t row, int col)
{
    if (g.drop.on) v = ws_drop1(v, g.drop, (unsigned long long)(row * g.dn + col));
    if (g.y) v *= g.y[row * g.ld + col] > 0.0f ? 1.0f : g.slope;
    if (g.mask) v = g.mask[row * g.ldm + col] ? v * g.mscale : 0.0f;
    return v;
}

__device__ __forceinline__ float4 ld4_guard(const float* __restrict__ p, int64_t row, int64_t nrows, int col, int ncols,
                                            int64_t ld, bool vec)
{
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < nrows) {
        const float* s = p + row * ld + col;
        if (vec && col + 3 < ncols) {
            v = *reinterpret_cast<const float4*>(s);
        } else {
            if (col + 0 < ncols) v.x = s[0];
            if (col + 1 < ncols) v.y = s[1];
            if (col + 2 < ncols) v.z = s[2];
            if (col + 3 < ncols) v.w = s[3];
        }
    }
    return v;
}

// ---- grouped launches: several mutually independent problems of ONE instantiation behind one grid -------------------------
// The group struct travels by value in the kernel arguments (at most GROUP_MAX problems, < 4 KB).  end[j] = workgroups of
// problems 0 .. j (running totals; entries past the last problem repeat the total).  A workgroup finds its problem with
// GROUP_MAX - 1 compares on blockIdx.x -- wave-uniform, like everything read from the descriptor (scalar loads, no private
// memory) -- takes its coordinates from that problem's OWN grid dimensions (x fastest, as the hardware deals a 3-D grid)
// and runs the single kernel's body: a member computes exactly what it computes launched alone.  No member waits for
// another: nothing is synchronised across workgroups.
struct GroupIndex { unsigned end[GROUP_MAX]; };
__device__ __forceinline__ int group_find(const GroupIndex& gi, unsigned& local)
{
    const unsigned b = blockIdx.x;
    int i = 0;
    unsigned beg = 0;
#pragma unroll
    for (int j = 0; j < GROUP_MAX - 1; ++j) {
        const bool past = b >= gi.end[j];
        i += past ? 1 : 0;
        beg = past ? gi.end[j] : beg;
    }
    local = b - beg;
    return i;
}
// running workgroup totals of a group: member j ends at end[j], entries past the last member repeat the total
struct GroupFill {
    GroupIndex& gi;
    int n = 0;
    unsigned total = 0;
    void add(unsigned blocks)
    {
        total += blocks;
        for (int j = n++; j < GROUP_MAX; ++j) gi.end[j] = total;
    }
};

}  // namespace
