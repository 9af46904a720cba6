// weasal_amd/csrc/gemm_xty.hip -- the kernels of O[K,N] = X[M,K]^T * Y[M,N] (dW: a reduction over the tall dimension) and
// their launchers: gemm_xty_kernel, gemm_xty2_kernel and its grouped form, and the chunk sums (reduce_partials_kernel, its wide
// and grouped forms -- also the column sums' of gemm_colsum.hip, through launch_reduce_partials).  Which of them a product takes
// is gemm.hip's xty_plan.  The f32-input MFMA and its lane maps: gemm.hip's header.
#include "gemm_device.h"

namespace {

// ---------------------------------------------------------------------------------------------
// partial[c][K,N] = X[rows of chunk c, K]^T * Y[rows of chunk c, N].  Workgroup = (32*KT) k-rows x
// (32*NT) columns of the output for one chunk of tall rows.  The 4 waves are KT k-tiles x RG = 4/KT
// row groups: for narrow X (K <= 32 / 64) the waves split the tall rows of every LDS tile instead of
// idling on zero padding, and their accumulators are summed through LDS at the end (fixed order).
// ---------------------------------------------------------------------------------------------
template <int NT, int KT>
__global__ __launch_bounds__(256) void gemm_xty_kernel(const float* __restrict__ x, int64_t m, int k, int64_t ldx,
                                                        const float* __restrict__ yy, int n, int64_t ldy,
                                                        float* __restrict__ partial, int64_t chunk, int vecx, int vecy)
{
    constexpr int BN = 32 * NT;
    constexpr int BKO = 32 * KT;   // output rows (= columns of X) per workgroup
    constexpr int RG = 4 / KT;     // row groups
    constexpr int XS_FLOATS = BK * BKO, YS_FLOATS = BK * BN;
    constexpr int RED_FLOATS = (RG > 1) ? KT * NT * 16 * 64 : 0;
    constexpr int LDS_FLOATS = (XS_FLOATS + YS_FLOATS) > RED_FLOATS ? (XS_FLOATS + YS_FLOATS) : RED_FLOATS;
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    float (*Xs)[BKO] = reinterpret_cast<float (*)[BKO]>(lds);
    float (*Ys)[BN] = reinterpret_cast<float (*)[BN]>(lds + XS_FLOATS);
    const int t = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int lane = t & 63;
    const int kt = wave % KT, rg = wave / KT;
    const int k0 = blockIdx.y * BKO;
    const int n0 = blockIdx.z * BN;
    const int64_t mbeg = (int64_t)blockIdx.x * chunk;
    const int64_t mend = mbeg + chunk < m ? mbeg + chunk : m;
    constexpr int XPT = (XS_FLOATS / 4 + 255) / 256;
    constexpr int YPT = (YS_FLOATS / 4 + 255) / 256;
    f32x16 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

    float4 xv[XPT], yv[YPT];
    auto load_tiles = [&](int64_t r0) {
#pragma unroll
        for (int i = 0; i < XPT; ++i) {
            const int idx = t + 256 * i;
            const int rr = idx / (BKO / 4), cc = (idx % (BKO / 4)) * 4;
            xv[i] = (rr < BK) ? ld4_guard(x, r0 + rr, mend, k0 + cc, k, ldx, vecx) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < YPT; ++i) {
            const int idx = t + 256 * i;
            const int rr = idx / (BN / 4), cc = (idx % (BN / 4)) * 4;
            yv[i] = (rr < BK) ? ld4_guard(yy, r0 + rr, mend, n0 + cc, n, ldy, vecy) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int i = 0; i < XPT; ++i) {
            const int idx = t + 256 * i;
            const int rr = idx / (BKO / 4), cc = (idx % (BKO / 4)) * 4;
            if (rr < BK) *reinterpret_cast<float4*>(&Xs[rr][cc]) = xv[i];
        }
#pragma unroll
        for (int i = 0; i < YPT; ++i) {
            const int idx = t + 256 * i;
            const int rr = idx / (BN / 4), cc = (idx % (BN / 4)) * 4;
            if (rr < BK) *reinterpret_cast<float4*>(&Ys[rr][cc]) = yv[i];
        }
    };

    load_tiles(mbeg);
    const int ai = kt * 32 + (lane & 31), kk = lane >> 5, bj = lane & 31;
    for (int64_t r0 = mbeg; r0 < mend; r0 += BK) {
        store_tiles();
        __syncthreads();
        if (r0 + BK < mend) load_tiles(r0 + BK);
#pragma unroll
        for (int ss = 0; ss < BK / 2 / RG; ++ss) {
            const int s = ss * RG + rg;
            const float a = Xs[2 * s + kk][ai];          // A[i = output row][k = tall index]
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const float bb = Ys[2 * s + kk][32 * i + bj];
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, acc[i], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    if (RG > 1) {
        // sum the row groups in order rg = 1, 2, 3 onto rg = 0 (layout [kt][i][r][lane])
        float* red = lds;
        for (int src = 1; src < RG; ++src) {
            if (rg == src) {
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) red[((kt * NT + i) * 16 + r) * 64 + lane] = acc[i][r];
            }
            __syncthreads();
            if (rg == 0) {
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][r] += red[((kt * NT + i) * 16 + r) * 64 + lane];
            }
            __syncthreads();
        }
    }
    if (rg == 0) {
        float* out = partial + (int64_t)blockIdx.x * k * n;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int col = n0 + 32 * i + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = k0 + kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (row < k && col < n) out[(int64_t)row * n + col] = acc[i][r];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// gemm_xty2: the same reduction with NO LDS staging.  For O = X^T Y both MFMA operands index the
// tall dimension with k: lane (idx, h) of a step supplies row r + h of X (A operand, i = X column)
// and of Y (B operand, j = Y column), so a wave can load its operands straight from global memory in
// MFMA layout -- lanes 0-31 read 32*KT contiguous floats of one row, lanes 32-63 of the next.
// A lane loads KT (NT) adjacent columns at once; column c0 + KT*idx + tk belongs to the interleaved
// tile tk, so one dwordx2 load feeds two tiles.  A wave owns (32 KT) x (32 NT) outputs; the 4 waves
// of a workgroup are WK x WN tiles x WR row groups (row groups are summed through LDS at the end,
// fixed order).  Loads run U steps ahead of the MFMAs; no barrier in the main loop.
// ---------------------------------------------------------------------------------------------
// TI = float, or bf16_t for the bf16-feature path: 2-byte operand loads widened exactly to f32 in registers (the
// products and sums stay fp32: dW is the fp32 master gradient).
template <int KT, typename TI>
__device__ __forceinline__ void xty_load_cols(__amdgpu_buffer_rsrc_t srd, int off, int soff, float (&out)[KT])
{
    if constexpr (sizeof(TI) == 4) {
        if constexpr (KT == 2) {
            const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(srd, off, soff, 0);
            out[0] = __uint_as_float(v.x);
            out[1] = __uint_as_float(v.y);
        } else {
            out[0] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(srd, off, soff, 0));
        }
    } else {
        if constexpr (KT == 2) {
            const unsigned v = __builtin_amdgcn_raw_buffer_load_b32(srd, off, soff, 0);
            out[0] = ws_bf_lo(v);
            out[1] = ws_bf_hi(v);
        } else {
            out[0] = ws_bf_lo((unsigned)(unsigned short)__builtin_amdgcn_raw_buffer_load_b16(srd, off, soff, 0));
        }
    }
}

template <int KT, int NT, int WK, int WN, typename TI>
__device__ __forceinline__ void gemm_xty2_body(const unsigned bx, const unsigned by, const unsigned bz,
                                               const TI* __restrict__ x, int64_t m, int k, int64_t ldx,
                                               const TI* __restrict__ yy, int n, int64_t ldy,
                                               float* __restrict__ partial, int64_t chunk)
{
    constexpr int ES = (int)sizeof(TI);
    constexpr int WR = 4 / (WK * WN);
    constexpr int U = 8;                                   // steps (row pairs) per block
    __shared__ float red[(WR > 1) ? WK * WN * KT * NT * 16 * 64 : 1];
    const int t = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int lane = t & 63;
    const int idx = lane & 31, h = lane >> 5;
    const int wr = wave / (WK * WN), wk = (wave / WN) % WK, wn = wave % WN;
    const int c0 = ((int)by * WK + wk) * (32 * KT);
    const int n0 = ((int)bz * WN + wn) * (32 * NT);
    const int64_t mbeg = (int64_t)bx * chunk;
    const int64_t mend = mbeg + chunk < m ? mbeg + chunk : m;

    f32x16 acc[KT][NT];
#pragma unroll
    for (int a = 0; a < KT; ++a)
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][i][r] = 0.0f;

    // columns past the end are clamped (their outputs are never stored); rows past the end are clamped
    // and the A operand zeroed
    int xc = c0 + KT * idx;
    xc = xc + KT <= k ? xc : (k - KT > 0 ? k - KT : 0);
    int yc = n0 + NT * idx;
    yc = yc + NT <= n ? yc : (n - NT > 0 ? n - NT : 0);
    // buffer addressing: one descriptor per operand covering this workgroup's rows (wave-uniform: built
    // from kernel arguments and blockIdx only), per-lane constant byte offset, the row advance in the
    // scalar offset -> no vector address arithmetic next to the MFMAs, and rows past the end of the
    // chunk read as 0 through the descriptor's bounds check (no tail code)
    const int64_t nrows = mend - mbeg;
    const auto xsrd = __builtin_amdgcn_make_buffer_rsrc(const_cast<TI*>(x + mbeg * ldx), 0,
                                                        (int)(((nrows - 1) * ldx + k) * ES), 0x00020000);
    const auto ysrd = __builtin_amdgcn_make_buffer_rsrc(const_cast<TI*>(yy + mbeg * ldy), 0,
                                                        (int)(((nrows - 1) * ldy + n) * ES), 0x00020000);
    const int xoff = (int)(h * ldx + xc) * ES, yoff = (int)(h * ldy + yc) * ES;
    const int xstep = (int)ldx * 2 * ES, ystep = (int)ldy * 2 * ES;      // bytes per step (two rows)
    float xa[2][U][KT], ya[2][U][NT];
    auto load_block = [&](int blk, int slot) {                 // blk = index of the 2U-row block in the chunk (uniform)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int step = blk * U + u;
            xty_load_cols<KT, TI>(xsrd, xoff, step * xstep, xa[slot][u]);
            xty_load_cols<NT, TI>(ysrd, yoff, step * ystep, ya[slot][u]);
        }
    };
    auto compute = [&](int slot) {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int a = 0; a < KT; ++a)
#pragma unroll
                    for (int i = 0; i < NT; ++i)
                        acc[a][i] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[slot][u][a], ya[slot][u][i], acc[a][i], 0, 0, 0);
    };
    // row group wr takes blocks wr, wr + WR, ... of 2U rows; two blocks per trip (static register slots)
    const int nblk = (int)((nrows + 2 * U - 1) / (2 * U));
    int blk = wr;
    if (blk < nblk) load_block(blk, 0);
    for (; blk < nblk; blk += 2 * WR) {
        if (blk + WR < nblk) load_block(blk + WR, 1);
        compute(0);
        if (blk + WR < nblk) {
            if (blk + 2 * WR < nblk) load_block(blk + 2 * WR, 0);
            compute(1);
        }
    }
    if (WR > 1) {
        // sum the row groups in order 1, 2, 3 onto group 0 (layout [wk][wn][a][i][r][lane])
        const int base = ((wk * WN + wn) * KT * NT) * 16 * 64;
        for (int src = 1; src < WR; ++src) {
            if (wr == src) {
#pragma unroll
                for (int a = 0; a < KT; ++a)
#pragma unroll
                    for (int i = 0; i < NT; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) red[base + ((a * NT + i) * 16 + r) * 64 + lane] = acc[a][i][r];
            }
            __syncthreads();
            if (wr == 0) {
#pragma unroll
                for (int a = 0; a < KT; ++a)
#pragma unroll
                    for (int i = 0; i < NT; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[a][i][r] += red[base + ((a * NT + i) * 16 + r) * 64 + lane];
            }
            __syncthreads();
        }
    }
    if (wr == 0) {
        float* out = partial + (int64_t)bx * k * n;
#pragma unroll
        for (int a = 0; a < KT; ++a)
            if constexpr (NT == 2) {
                // the two interleaved column tiles of a lane are adjacent columns: one 8-byte store per row (a wave
                // instruction writes two full 256-byte row segments) when the row pitch allows it
                const int col = n0 + 2 * idx;
                if ((n & 1) == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = c0 + KT * ((r & 3) + 8 * (r >> 2) + 4 * h) + a;
                        if (row < k && col + 1 < n)
                            *reinterpret_cast<float2*>(out + (int64_t)row * n + col) = make_float2(acc[a][0][r], acc[a][1][r]);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < NT; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = c0 + KT * ((r & 3) + 8 * (r >> 2) + 4 * h) + a;
                            if (row < k && col + i < n) out[(int64_t)row * n + col + i] = acc[a][i][r];
                        }
                }
            } else {
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    const int col = n0 + NT * idx + i;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = c0 + KT * ((r & 3) + 8 * (r >> 2) + 4 * h) + a;
                        if (row < k && col < n) out[(int64_t)row * n + col] = acc[a][i][r];
                    }
                }
            }
    }
}

template <int KT, int NT, int WK, int WN, typename TI = float>
__global__ __launch_bounds__(256) void gemm_xty2_kernel(const TI* __restrict__ x, int64_t m, int k, int64_t ldx,
                                                         const TI* __restrict__ yy, int n, int64_t ldy,
                                                         float* __restrict__ partial, int64_t chunk)
{
    gemm_xty2_body<KT, NT, WK, WN, TI>(blockIdx.x, blockIdx.y, blockIdx.z, x, m, k, ldx, yy, n, ldy, partial, chunk);
}

// grouped form (f32 rows): see gemm_xb2_group_kernel
struct Xty2Problem {
    const float* x; int64_t m; int64_t ldx; const float* y; int64_t ldy; float* partial; int64_t chunk;
    int k, n; unsigned gx, gy;
};
struct Xty2Group { GroupIndex gi; Xty2Problem p[GROUP_MAX]; };
template <int KT, int NT, int WK, int WN>
__global__ __launch_bounds__(256) void gemm_xty2_group_kernel(const Xty2Group g)
{
    unsigned l;
    const Xty2Problem& p = g.p[group_find(g.gi, l)];
    const unsigned gx = p.gx, gy = p.gy;
    const unsigned bx = l % gx, q = l / gx;
    gemm_xty2_body<KT, NT, WK, WN, float>(bx, q % gy, q / gy, p.x, p.m, p.k, p.ldx, p.y, p.n, p.ldy, p.partial, p.chunk);
}

// out[e] = sum_c partial[c][e] in a fixed order (bitwise reproducible): 32 elements x 8 chunk groups
// per workgroup, group g adds chunks g, g+8, ... (coalesced 128-byte reads), then the 8 group sums
// are added in order.
// (n, ldo: the output is [elems / n, n] with row pitch ldo; ldo == n = flat)
__device__ __forceinline__ void reduce_partials_body(const unsigned bx, const float* __restrict__ partial, int64_t elems, int chunks,
                                                     float* __restrict__ out, int n, int64_t ldo)
{
    __shared__ float red[8][32];
    const int el = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const int64_t e = (int64_t)bx * 32 + el;
    float s = 0.0f;
    if (e < elems) {
        int c = grp;
        for (; c + 24 < chunks; c += 32) {                 // four loads in flight, added in order
            const float v0 = partial[(int64_t)c * elems + e], v1 = partial[(int64_t)(c + 8) * elems + e];
            const float v2 = partial[(int64_t)(c + 16) * elems + e], v3 = partial[(int64_t)(c + 24) * elems + e];
            s += v0; s += v1; s += v2; s += v3;
        }
        for (; c < chunks; c += 8) s += partial[(int64_t)c * elems + e];
    }
    red[grp][el] = s;
    __syncthreads();
    if (grp == 0 && e < elems) {
        float t = red[0][el];
#pragma unroll
        for (int g2 = 1; g2 < 8; ++g2) t += red[g2][el];
        out[ldo > n ? (e / n) * ldo + e % n : e] = t;
    }
}

__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ partial, int64_t elems, int chunks,
                                                               float* __restrict__ out, int n = 0, int64_t ldo = 0)
{
    reduce_partials_body(blockIdx.x, partial, elems, chunks, out, n, ldo);
}

// the same sum for LARGE outputs of few chunks (dW of the deep levels: k n up to 4 M elements, <= ~16 chunks): a thread owns
// four consecutive elements and adds the chunks in order 0, 1, 2, ... (four 16-byte loads in flight)
__device__ __forceinline__ void reduce_partials_wide_body(const unsigned bx, const float* __restrict__ partial, int64_t elems, int chunks,
                                                          float* __restrict__ out, int n, int64_t ldo)
{
    const int64_t e = ((int64_t)bx * 256 + threadIdx.x) * 4;
    if (e >= elems) return;
    const float4* p = reinterpret_cast<const float4*>(partial + e);
    const int64_t st = elems / 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    int c = 0;
    for (; c + 3 < chunks; c += 4) {
        const float4 v0 = p[(int64_t)c * st], v1 = p[(int64_t)(c + 1) * st], v2 = p[(int64_t)(c + 2) * st], v3 = p[(int64_t)(c + 3) * st];
        s.x += v0.x; s.y += v0.y; s.z += v0.z; s.w += v0.w;
        s.x += v1.x; s.y += v1.y; s.z += v1.z; s.w += v1.w;
        s.x += v2.x; s.y += v2.y; s.z += v2.z; s.w += v2.w;
        s.x += v3.x; s.y += v3.y; s.z += v3.z; s.w += v3.w;
    }
    for (; c < chunks; ++c) {
        const float4 v = p[(int64_t)c * st];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *reinterpret_cast<float4*>(out + (ldo > n ? (e / n) * ldo + e % n : e)) = s;      // (n % 4 == 0: a quad stays in its row)
}

__global__ __launch_bounds__(256) void reduce_partials_wide_kernel(const float* __restrict__ partial, int64_t elems, int chunks,
                                                                    float* __restrict__ out, int n = 0, int64_t ldo = 0)
{
    reduce_partials_wide_body(blockIdx.x, partial, elems, chunks, out, n, ldo);
}

// the chunk sums of a grouped gemm_xty2 launch: member j runs the form it takes alone (wide: reduce_partials_wide_kernel's
// body, else reduce_partials_kernel's; the choice is uniform over a workgroup) over the workgroups it takes alone
struct ReduceProblem { const float* partial; int64_t elems; float* out; int64_t ldo; int chunks, n, wide; };
struct ReduceGroup { GroupIndex gi; ReduceProblem p[GROUP_MAX]; };
__global__ __launch_bounds__(256) void reduce_partials_group_kernel(const ReduceGroup g)
{
    unsigned l;
    const ReduceProblem& p = g.p[group_find(g.gi, l)];
    if (p.wide) reduce_partials_wide_body(l, p.partial, p.elems, p.chunks, p.out, p.n, p.ldo);
    else reduce_partials_body(l, p.partial, p.elems, p.chunks, p.out, p.n, p.ldo);
}

int xty2_no_instantiation(const XtyPlan& p)
{
    return ws_no_instantiation("gemm_xty2_kernel<KT=%d, NT=%d, WK=%d, WN=%d> bf16=%d", p.kt, p.nt, p.wk, p.wn, p.bf16);
}

}  // namespace

namespace gemm {

// chunk sums -> out (also gemm.hip's column sums): the wide form for large outputs of few chunks (gemm.hip's
// reduce_partials_wide decides), the grouped form otherwise
void launch_reduce_partials(bool wide, const float* partial, int64_t elems, int chunks, float* out, hipStream_t st, int n, int64_t ldo)
{
    if (wide)
        reduce_partials_wide_kernel<<<(unsigned)ws_ceil_div(elems, 1024), 256, 0, st>>>(partial, elems, chunks, out, n, ldo);
    else
        reduce_partials_kernel<<<(unsigned)ws_ceil_div(elems, 32), 256, 0, st>>>(partial, elems, chunks, out, n, ldo);
}

// gemm_xty2_kernel: a product alone (f32 or bf16 rows), and a grouped member nobody shares an instantiation with
int launch_xty2(const ws_xty_problem& q, const XtyPlan& p, hipStream_t st)
{
    const bool called = dispatch([&](auto bf, auto kt, auto nt, auto wk, auto wn) {
        using T = Row<bf.value>;
        gemm_xty2_kernel<kt.value, nt.value, wk.value, wn.value, T><<<p.grid, 256, 0, st>>>((const T*)q.x, q.m, q.k, q.ldx, (const T*)q.y, q.n,
                                                                                           q.ldy, p.partial, p.chunk);
    }, Flag{p.bf16}, Pick<1, 2>{p.kt}, Pick<1, 2>{p.nt}, Pick<1, 2>{p.wk}, Pick<1, 2>{p.wn});
    return called ? WS_OK : xty2_no_instantiation(p);
}

int launch_xty_lds(const ws_xty_problem& q, const XtyPlan& p, hipStream_t st)
{
    const bool called = dispatch([&](auto nt, auto kt) {
        gemm_xty_kernel<nt.value, kt.value><<<p.grid, 256, 0, st>>>(q.x, q.m, q.k, q.ldx, q.y, q.n, q.ldy, p.partial, p.chunk, p.vecx, p.vecy);
    }, Pick<1, 2, 4>{p.nt}, Pick<1, 2, 4>{p.kt});
    return called ? WS_OK : ws_no_instantiation("gemm_xty_kernel<NT=%d, KT=%d>", p.nt, p.kt);
}

// members ids[0 .. cnt) of one instantiation (gemm.hip's bucket) behind one grid
int launch_xty2_group(const ws_xty_problem* q, const XtyPlan* plan, const int* ids, int cnt, hipStream_t st)
{
    Xty2Group g{};
    GroupFill gf{g.gi};
    for (int j = 0; j < cnt; ++j) {
        const ws_xty_problem& a = q[ids[j]];
        const XtyPlan& p = plan[ids[j]];
        g.p[j] = Xty2Problem{a.x, a.m, a.ldx, a.y, a.ldy, p.partial, p.chunk, a.k, a.n, p.grid.x, p.grid.y};
        gf.add(p.grid.x * p.grid.y * p.grid.z);
    }
    const XtyPlan& p0 = plan[ids[0]];
    const bool called = dispatch([&](auto kt, auto nt, auto wk, auto wn) {
        gemm_xty2_group_kernel<kt.value, nt.value, wk.value, wn.value><<<gf.total, 256, 0, st>>>(g);
    }, Pick<1, 2>{p0.kt}, Pick<1, 2>{p0.nt}, Pick<1, 2>{p0.wk}, Pick<1, 2>{p0.wn});
    return called ? WS_OK : xty2_no_instantiation(p0);
}

// the chunk sums of members ids[0 .. cnt) (each plan's reduce != 0) behind one grid
void launch_reduce_group(const ws_xty_problem* q, const XtyPlan* plan, const int* ids, int cnt, hipStream_t st)
{
    ReduceGroup g{};
    GroupFill gf{g.gi};
    for (int j = 0; j < cnt; ++j) {
        const ws_xty_problem& a = q[ids[j]];
        const XtyPlan& p = plan[ids[j]];
        const int64_t elems = (int64_t)a.k * a.n;
        g.p[j] = ReduceProblem{p.partial, elems, a.out, p.pitched ? a.ldo : 0, p.chunks, a.n, p.reduce == 2 ? 1 : 0};
        gf.add((unsigned)ws_ceil_div(elems, p.reduce == 2 ? 1024 : 32));
    }
    reduce_partials_group_kernel<<<gf.total, 256, 0, st>>>(g);
}

}  // namespace gemm
