// weasal_amd/csrc/gemm.hip -- tall-skinny fp32 GEMMs on the f32-input MFMA (v_mfma_f32_32x32x2_f32).
//
// The dense parts of the KPConv hot path are all "M huge, K and N small":
//   the per-point unary MLPs            y = x W^T            (models/blocks.py:490-501, nn.Linear)
//   the kernel contraction               out = wf [N,15Ci] x weights [15Ci,Co]   (blocks.py:370-374)
// and their autograd (dx = dy W, dW = dy^T x).  With M = 400 000 rows and N,K in 32..512 they are
// bound by streaming the tall operand once; rocBLAS's fp32 solutions for these shapes run at a
// few % of that (profiles/r01_*).  Two kernels cover everything:
//
//   gemm_xb  : Y[M,N]  = X[M,K] * B[K,N]        B row-major, small.  (forward and dX)
//   gemm_xty : O[K,N]  = X[M,K]^T * Y[M,N]      reduction over the tall dimension.  (dW)
//
// Both stage 32-deep tiles in LDS with coalesced 16-byte loads (register prefetch of the next
// tile under the MFMAs of the current one) and feed v_mfma_f32_32x32x2_f32: exact fp32 (one
// rounding per product, a k-ordered fma chain), so results differ from rocBLAS only by summation
// order.  A operand lane map: A[i = lane&31][k = lane>>5]; B: B[k = lane>>5][j = lane&31];
// C/D: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)  (cdna_hip_programming.md section 3).
#include "ws_common.h"
#include "ws_dispatch.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128;   // rows of X per workgroup (32 per wave)
constexpr int BK = 32;    // k depth per LDS tile

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

// ---------------------------------------------------------------------------------------------
// Y[M,N] = X[M,K] * B[K,N].  Workgroup = 4 waves = 128 rows x (32*NT) columns; wave w owns rows
// 32w..32w+31 and NT accumulator tiles.
// ---------------------------------------------------------------------------------------------
template <int NT, int BKX>
__global__ __launch_bounds__(256) void gemm_xb_kernel(const float* __restrict__ x, int64_t m, int k, int64_t ldx,
                                                       const float* __restrict__ b, int n, int64_t ldb,
                                                       float* __restrict__ y, int64_t ldy, int vecx, int vecb,
                                                       const float* __restrict__ bias, const float* __restrict__ residual,
                                                       int64_t ldr, int act, float slope, const XbGate gate)
{
    constexpr int BN = 32 * NT;
    __shared__ float Xs[BM][BKX + 1];
    __shared__ __attribute__((aligned(16))) float Bs[BKX][BN];
    const int t = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int lane = t & 63;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    constexpr int XCOLS4 = BKX / 4;                      // float4 per X-tile row
    constexpr int XROWS = 256 / XCOLS4;                  // rows covered by one pass of the 256 threads
    constexpr int XPT = BM / XROWS;                      // passes
    const int xr = t / XCOLS4, xc = (t % XCOLS4) * 4;    // X tile: rows xr + XROWS i, cols xc..xc+3
    constexpr int BPT = (BKX * BN / 4 + 255) / 256;      // float4 of the B tile per thread
    f32x16 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

    float4 xv[XPT], bv[BPT];
    auto load_tiles = [&](int k0) {
#pragma unroll
        for (int i = 0; i < XPT; ++i) xv[i] = ld4_guard(x, m0 + xr + XROWS * i, m, k0 + xc, k, ldx, vecx);
#pragma unroll
        for (int i = 0; i < BPT; ++i) {
            const int idx = t + 256 * i;
            const int br = idx / (BN / 4), bc = (idx % (BN / 4)) * 4;
            bv[i] = (br < BKX) ? ld4_guard(b, k0 + br, k, n0 + bc, n, ldb, vecb) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int i = 0; i < XPT; ++i) {
            float* d = &Xs[xr + XROWS * i][xc];
            d[0] = xv[i].x; d[1] = xv[i].y; d[2] = xv[i].z; d[3] = xv[i].w;
        }
#pragma unroll
        for (int i = 0; i < BPT; ++i) {
            const int idx = t + 256 * i;
            const int br = idx / (BN / 4), bc = (idx % (BN / 4)) * 4;
            if (br < BKX) *reinterpret_cast<float4*>(&Bs[br][bc]) = bv[i];
        }
    };

    load_tiles(0);
    const int ai = wave * 32 + (lane & 31), kk = lane >> 5, bj = lane & 31;
    for (int k0 = 0; k0 < k; k0 += BKX) {
        store_tiles();
        __syncthreads();
        if (k0 + BKX < k) load_tiles(k0 + BKX);    // in flight under the MFMAs below
#pragma unroll
        for (int s = 0; s < BKX / 2; ++s) {
            const float a = Xs[ai][2 * s + kk];
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const float bb = Bs[2 * s + kk][32 * i + bj];
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, acc[i], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // epilogue (+ bias[col], + residual[row,col], LeakyReLU): 32 lanes write 128 contiguous bytes of one row
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int col = n0 + 32 * i + (lane & 31);
        const float bv = (bias && col < n) ? bias[col] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (row < m && col < n) {
                float v = acc[i][r] + bv;
                if (residual) { const float* rr_ = xb_res_row(residual, ldr, gate, row); if (rr_) v += rr_[col]; }
                if (act) v = v > 0.0f ? v : v * slope;
                y[row * ldy + col] = xb_gate1(v, gate, row, col);
            }
        }
    }
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// shared float4 epilogue of the rows-on-lanes kernels: lane = row, register quad g of tile i = columns
// n0 + 32 i + 8 g + 4 h .. + 3.  Residual quads are loaded with clamped columns (no control flow around
// the loads, so they are all in flight together); only the stores are predicated.
template <int NT>
__device__ __forceinline__ void xb_rows_epilogue(const f32x16 (&acc)[NT], int64_t row, int64_t m, int n0, int n, int h,
                                                 float* __restrict__ y, int64_t ldy, const float* __restrict__ bias,
                                                 const float* __restrict__ residual, int64_t ldr, int act, float slope,
                                                 const XbGate& gate)
{
    const bool live = row < m;
    const int64_t rr = live ? row : m - 1;
    float* yrow = y + rr * ldy;
    const float* rrow = xb_res_row(residual, ldr, gate, rr);
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        float4 v[4];
        int col[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            col[g] = n0 + 32 * i + 8 * g + 4 * h;
            v[g] = make_float4(acc[i][4 * g + 0], acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3]);
        }
        if (rrow) {
            float4 rq[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) rq[g] = *reinterpret_cast<const float4*>(rrow + (col[g] < n ? col[g] : n - 4));
#pragma unroll
            for (int g = 0; g < 4; ++g) { v[g].x += rq[g].x; v[g].y += rq[g].y; v[g].z += rq[g].z; v[g].w += rq[g].w; }
        }
        if (bias) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 bq = *reinterpret_cast<const float4*>(bias + (col[g] < n ? col[g] : n - 4));
                v[g].x += bq.x; v[g].y += bq.y; v[g].z += bq.z; v[g].w += bq.w;
            }
        }
        if (act) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                v[g].x = v[g].x > 0.0f ? v[g].x : v[g].x * slope;
                v[g].y = v[g].y > 0.0f ? v[g].y : v[g].y * slope;
                v[g].z = v[g].z > 0.0f ? v[g].z : v[g].z * slope;
                v[g].w = v[g].w > 0.0f ? v[g].w : v[g].w * slope;
            }
        }
        if (gate.y || gate.mask || gate.drop.on) {
#pragma unroll
            for (int g = 0; g < 4; ++g) xb_gate4(v[g], gate, rr, col[g] < n ? col[g] : n - 4);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g)
            if (live && col[g] < n) *reinterpret_cast<float4*>(yrow + col[g]) = v[g];
    }
}

// The same epilogue with the wave's 32 x 32 tile turned through LDS first.  In the rows-on-lanes layout a store instruction
// writes 16 bytes to each of 32 DIFFERENT rows (two column quads): a row's 128-byte line is completed by four separate
// instructions, and residual rows are read the same way -- products whose traffic is their output (K = 32 .. 64) ran at
// 2.5-3.3 TB/s where read-dominated ones reach 4.4-5.2.  Staged: lane (r = lane / 8, c = lane % 8)
// owns the float4 at row r + 8 p, columns 4 c .. 4 c + 3 of the tile: one instruction moves 8 whole 128-byte row segments.
// `stage`: wave-private [32][36] floats (the W buffers, free after the main loop).
constexpr int XB_STAGE_LD = 36;
constexpr int XB_STAGE_FLOATS = 32 * XB_STAGE_LD;
template <int NT>
__device__ __forceinline__ void xb_rows_epilogue_staged(const f32x16 (&acc)[NT], int64_t row0, int64_t m, int n0, int n, int lane,
                                                        float* __restrict__ y, int64_t ldy, const float* __restrict__ bias,
                                                        const float* __restrict__ residual, int64_t ldr, int act, float slope,
                                                        const XbGate& gate, float* __restrict__ stage)
{
    const int idx = lane & 31, h = lane >> 5;
    const int r8 = lane >> 3, c4 = lane & 7;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4*>(&stage[idx * XB_STAGE_LD + 8 * g + 4 * h]) =
                make_float4(acc[i][4 * g + 0], acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        const int col = n0 + 32 * i + 4 * c4;
        const int colc = col < n ? col : n - 4;
        float4 bq = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bias) bq = *reinterpret_cast<const float4*>(bias + colc);
        float4 v[4], rq[4];
        int64_t rr[4];
        bool live[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int rl = r8 + 8 * p;
            const int64_t row = row0 + rl;
            live[p] = row < m && col < n;
            rr[p] = row < m ? row : m - 1;
            v[p] = *reinterpret_cast<const float4*>(&stage[rl * XB_STAGE_LD + 4 * c4]);
            rq[p] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (residual) {
                const float* rrow = xb_res_row(residual, ldr, gate, rr[p]);
                if (rrow) rq[p] = *reinterpret_cast<const float4*>(rrow + colc);
            }
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            v[p].x = (v[p].x + rq[p].x) + bq.x; v[p].y = (v[p].y + rq[p].y) + bq.y;      // residual first, then bias: the order of
            v[p].z = (v[p].z + rq[p].z) + bq.z; v[p].w = (v[p].w + rq[p].w) + bq.w;      // xb_rows_epilogue (bit-identical results)
            if (act) {
                v[p].x = v[p].x > 0.0f ? v[p].x : v[p].x * slope;
                v[p].y = v[p].y > 0.0f ? v[p].y : v[p].y * slope;
                v[p].z = v[p].z > 0.0f ? v[p].z : v[p].z * slope;
                v[p].w = v[p].w > 0.0f ? v[p].w : v[p].w * slope;
            }
            if (gate.y || gate.mask || gate.drop.on) xb_gate4(v[p], gate, rr[p], colc);
            if (live[p]) *reinterpret_cast<float4*>(y + rr[p] * ldy + col) = v[p];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    }
}

// ---------------------------------------------------------------------------------------------
// gemm_xb2: same product, "rows on the lanes".  The MFMA is fed transposed: A operand = the small
// matrix (i = output column), B operand = X (j = row of X), so that
//   * X never goes through LDS: lane (idx, h) reads float4 X[row idx][k0 + 8j + 4h ..] straight into
//     the B-operand registers (a row's 128-byte line is consumed by 4 consecutive loads of one wave);
//     MFMA step (j, e) contracts k = k0 + 8j + 4h + e, the two wave halves supplying two different k;
//   * the small matrix chunk [32 x BN] is staged in LDS already interleaved as Ws[t][j][h][idx][e], so
//     one conflict-free ds_read_b128 feeds four MFMAs; double buffered: ONE barrier per 32-deep chunk;
//   * a lane ends up with 4 consecutive output columns of its own row per register quad: the epilogue
//     is float4 (bias, residual, LeakyReLU, store) instead of 16 scalar stores per tile.
// Workgroup = 4 waves, wave w owns RT row tiles of 32 rows, all waves share the W chunk.
// ---------------------------------------------------------------------------------------------
// Preconditions (checked by the launcher; everything else takes gemm_xb_kernel): k % 32 == 0, n % 4 == 0,
// x / y / residual rows 16-byte aligned.  Rows past m and columns past n are clamped on the loads
// (valid memory, results never stored), so the main loop has no divergent control flow at all.
// The body runs for workgroup (bx, by, bz) of ONE product's own grid: gemm_xb2_kernel passes blockIdx, the grouped kernel
// (gemm_xb2_group_kernel) the coordinates it derives from a linear index -- everything else is the same code.
template <int NT, int WN>
__device__ __forceinline__ void gemm_xb2_body(
    const unsigned bx, const unsigned by, const unsigned bz,
    const float* __restrict__ x, int64_t m, int k, int64_t ldx, const float* __restrict__ b, int n, int ldb, int bcs,
    float* __restrict__ y, int64_t ldy, const float* __restrict__ bias, const float* __restrict__ residual, int64_t ldr,
    int act, float slope, int csplit, float* __restrict__ partial, const XbGate& gate, int staged)
{
    // split-K (gridDim.z > 1; few rows, deep k): workgroup z contracts chunks [z*csplit, (z+1)*csplit) and
    // writes its raw sums to partial[z][m][n]; splitk_epilogue_kernel adds them in a fixed order
    constexpr int WM = 4 / WN;                            // wave grid WM x WN: rows x column groups
    constexpr int CT = NT * WN;                           // 32-column tiles per workgroup
    constexpr int BN = 32 * CT;
    constexpr int KC = 32;
    constexpr int WBUF = CT * 1024;                       // floats per W chunk buffer
    constexpr int WS_FLOATS = 2 * WBUF > 4 * XB_STAGE_FLOATS ? 2 * WBUF : 4 * XB_STAGE_FLOATS;
    __shared__ __attribute__((aligned(16))) float Ws[WS_FLOATS];
    const int t = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int lane = t & 63;
    const int idx = lane & 31, h = lane >> 5;
    const int64_t row = (int64_t)bx * (32 * WM) + wm * 32 + idx;
    const int n0 = by * BN;
    const int cbeg = bz * csplit;
    const int cend = (cbeg + csplit) * KC < k ? cbeg + csplit : k / KC;

    f32x16 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

    // W staging: group g = t + 256 i -> column c = g % BN, row quad q = g / BN (rows 4q .. 4q+3 of the
    // chunk) -> one float4 at Ws[tile = c/32][j = q/2][h = q%2][idx = c%32][e = 0..3]
    // buffer addressing (wave-uniform descriptors from kernel arguments / blockIdx, per-lane constant byte
    // offsets, the chunk advance in the scalar offset): no vector address arithmetic in the loop; rows of
    // X past m read as 0 through the bounds check
    // B[kk][col] = b[kk * ldb + col * bcs]: bcs = 1 is the row-major [K,N] matrix, ldb = 1 with bcs = K' reads a
    // row-major [N,K'] matrix as its transpose (nn.Linear's weight, or a weight's transpose in a backward) in place
    const auto wsrd = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(b), 0,
                                                        (int)(((int64_t)(k - 1) * ldb + (int64_t)(n - 1) * bcs + 1) * 4), 0x00020000);
    const int64_t brow0 = (int64_t)bx * (32 * WM);
    const int64_t brows = m - brow0 < 32 * WM ? m - brow0 : 32 * WM;
    const auto xsrd = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x + brow0 * ldx), 0,
                                                        (int)(((brows - 1) * ldx + k) * 4), 0x00020000);
    int woff[CT];
    int wlds[CT];
    // transposed-in-place small matrix (ldb == 1): the four k of a row quad are 16 contiguous bytes and the 8 quads of a
    // chunk one 128-byte line per column -> lanes run along k (8 lanes per column, one dwordx4 each: 8 whole lines per wave
    // instruction); row-major: lanes run along the columns, four dword loads one row apart
    const bool wtr = ldb == 1;
#pragma unroll
    for (int i = 0; i < CT; ++i) {
        const int g = t + 256 * i;
        const int c = wtr ? g / 8 : g % BN, q = wtr ? g % 8 : g / BN;
        int col = n0 + c;
        col = col < n ? col : n - 1;
        woff[i] = (4 * q * ldb + col * bcs) * 4;
        wlds[i] = ((((c >> 5) * 4 + (q >> 1)) * 2 + (q & 1)) * 32 + (c & 31)) * 4;
    }
    float4 wv[CT];
    auto load_w = [&](int chunk) {
        const int so = chunk * KC * ldb * 4;                       // uniform byte offset of the chunk
        if (wtr) {
#pragma unroll
            for (int i = 0; i < CT; ++i) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(wsrd, woff[i], so, 0);
                wv[i] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < CT; ++i) {
            wv[i].x = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wsrd, woff[i], so, 0));
            wv[i].y = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wsrd, woff[i], so + ldb * 4, 0));
            wv[i].z = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wsrd, woff[i], so + ldb * 8, 0));
            wv[i].w = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wsrd, woff[i], so + ldb * 12, 0));
        }
    };
    auto store_w = [&](int buf) {
#pragma unroll
        for (int i = 0; i < CT; ++i) *reinterpret_cast<float4*>(&Ws[buf * WBUF + wlds[i]]) = wv[i];
    };
    const int xoff = (int)((wm * 32 + idx) * ldx + 4 * h) * 4;
    float4 xn[4], xc[4];
    auto load_x = [&](int chunk) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(xsrd, xoff + 32 * j, chunk * (KC * 4), 0);
            xn[j] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
        }
    };

    const int last = cend - 1;
    load_w(cbeg);
    load_x(cbeg);
    {   // chunk 1 of W goes out before anything waits on chunk 0
        float4 w0[CT];
#pragma unroll
        for (int i = 0; i < CT; ++i) w0[i] = wv[i];
        load_w(last < cbeg + 1 ? last : cbeg + 1);
#pragma unroll
        for (int i = 0; i < CT; ++i) *reinterpret_cast<float4*>(&Ws[wlds[i]]) = w0[i];
    }
    __syncthreads();
    for (int c = cbeg; c < cend; ++c) {
#pragma unroll
        for (int j = 0; j < 4; ++j) xc[j] = xn[j];
        store_w((c - cbeg + 1) & 1);                            // chunk c+1 (a harmless repeat after the last one)
        load_x(c + 1 < last ? c + 1 : last);
        load_w(c + 2 < last ? c + 2 : last);
        const float* wb = &Ws[((c - cbeg) & 1) * WBUF + wn * (NT * 1024) + (h * 32 + idx) * 4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            __builtin_amdgcn_sched_barrier(0);   // keep the LDS reads of step j+1 out of step j (registers)
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const float4 a4 = *reinterpret_cast<const float4*>(wb + (i * 4 + j) * 256);
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, xc[j].x, acc[i], 0, 0, 0);
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, xc[j].y, acc[i], 0, 0, 0);
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, xc[j].z, acc[i], 0, 0, 0);
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, xc[j].w, acc[i], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    if (staged) {
        // (the main loop ended on a barrier: nobody reads the W buffers any more)
        const int64_t row0 = (int64_t)bx * (32 * WM) + wm * 32;
        float* stage = &Ws[wave * XB_STAGE_FLOATS];
        if (partial)
            xb_rows_epilogue_staged<NT>(acc, row0, m, n0 + wn * (32 * NT), n, lane, partial + (int64_t)bz * m * n, n, nullptr,
                                        nullptr, 0, 0, 0.0f, XbGate{}, stage);
        else
            xb_rows_epilogue_staged<NT>(acc, row0, m, n0 + wn * (32 * NT), n, lane, y, ldy, bias, residual, ldr, act, slope, gate, stage);
        return;
    }
    if (partial)
        xb_rows_epilogue<NT>(acc, row, m, n0 + wn * (32 * NT), n, h, partial + (int64_t)bz * m * n, n, nullptr, nullptr, 0,
                             0, 0.0f, XbGate{});
    else
        xb_rows_epilogue<NT>(acc, row, m, n0 + wn * (32 * NT), n, h, y, ldy, bias, residual, ldr, act, slope, gate);
}

template <int NT, int WN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void gemm_xb2_kernel(
    const float* __restrict__ x, int64_t m, int k, int64_t ldx, const float* __restrict__ b, int n, int ldb, int bcs,
    float* __restrict__ y, int64_t ldy, const float* __restrict__ bias, const float* __restrict__ residual, int64_t ldr,
    int act, float slope, int csplit, float* __restrict__ partial, const XbGate gate, int staged)
{
    gemm_xb2_body<NT, WN>(blockIdx.x, blockIdx.y, blockIdx.z, x, m, k, ldx, b, n, ldb, bcs, y, ldy, bias, residual, ldr, act, slope,
                          csplit, partial, gate, staged);
}

// ---- grouped launches: several mutually independent problems of ONE instantiation behind one grid -------------------------
// The group struct travels by value in the kernel arguments (at most GROUP_MAX problems, < 4 KB).  end[j] = workgroups of
// problems 0 .. j (running totals; entries past the last problem repeat the total).  A workgroup finds its problem with
// GROUP_MAX - 1 compares on blockIdx.x -- wave-uniform, like everything read from the descriptor (scalar loads, no private
// memory) -- takes its coordinates from that problem's OWN grid dimensions (x fastest, as the hardware deals a 3-D grid)
// and runs the single kernel's body: a member computes exactly what it computes launched alone.  No member waits for
// another: nothing is synchronised across workgroups.
constexpr int GROUP_MAX = 8;
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

struct Xb2Problem {
    const float* x; int64_t m; int64_t ldx; const float* b; float* y; int64_t ldy; const float* bias; const float* residual;
    int64_t ldr; float* partial; XbGate gate;
    int k, n, ldb, bcs, act, csplit, staged; float slope;
    unsigned gx, gy;        // the problem's own grid (x, y); z = local / (gx * gy)
};
struct Xb2Group { GroupIndex gi; Xb2Problem p[GROUP_MAX]; };
static_assert(sizeof(Xb2Group) < 4096, "the group travels in the kernel arguments");

template <int NT, int WN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void gemm_xb2_group_kernel(const Xb2Group g)
{
    unsigned l;
    const Xb2Problem& p = g.p[group_find(g.gi, l)];
    const unsigned gx = p.gx, gy = p.gy;
    const unsigned bx = l % gx, q = l / gx;
    gemm_xb2_body<NT, WN>(bx, q % gy, q / gy, p.x, p.m, p.k, p.ldx, p.b, p.n, p.ldb, p.bcs, p.y, p.ldy, p.bias, p.residual, p.ldr,
                          p.act, p.slope, p.csplit, p.partial, p.gate, p.staged);
}

// ---------------------------------------------------------------------------------------------
// gemm_xb_shallow: Y = act(X [m, k] @ B [k, n] + bias + residual) for contractions too shallow and ragged for the MFMA tiles
// (k = 9: the logits' dX; k = 45: the 3-channel input layer's contraction).  The arithmetic is nothing (k FMAs per output); what
// matters is that the output -- all of the traffic -- leaves as whole 128-byte row segments and that the epilogue menu
// (residual, bias, LeakyReLU, gates) is the float4 one.  Thread = 4 consecutive columns of one row: the k values of its row
// come from L1 (the n / 4 threads of a row read the same addresses), the 4 columns of B from LDS (one ds_read_b128 per k,
// the same address for all rows of a wave's column); sequential fmaf over k (fixed order).  gemm_xb_kernel's scalar
// epilogue took 90-96 us on these shapes at M = 400 000, 3-4 x their streaming time.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gemm_xb_shallow_kernel(const float* __restrict__ x, int64_t m, int k, int64_t ldx,
                                                               const float* __restrict__ b, int n, float* __restrict__ y, int64_t ldy,
                                                               const float* __restrict__ bias, const float* __restrict__ residual,
                                                               int64_t ldr, int act, float slope, const XbGate gate, int rows_per_wg)
{
    // LDS: B as [kp][n] (kp = k rounded up to 4, the extra rows zero) and the workgroup's rows of X as [rows_per_wg][kp] (each
    // element of X loaded once, coalesced; a thread then takes four k of its row per ds_read_b128 -- through global loads the
    // n / 4 threads of a row each issued the same k dword loads: address-unit bound, 121 us on the 45-deep shape)
    extern __shared__ __attribute__((aligned(16))) float shallow_lds[];
    const int kp = (k + 3) & ~3;
    float* bs = shallow_lds;
    float* xs = shallow_lds + kp * n;
    const int t = threadIdx.x;
    for (int e = t; e < kp * n / 4; e += 256)
        reinterpret_cast<float4*>(bs)[e] = e < k * n / 4 ? reinterpret_cast<const float4*>(b)[e] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
    const int64_t r1 = r0 + rows_per_wg < m ? r0 + rows_per_wg : m;
    const int nrows = (int)(r1 - r0);
    {   // (row, k) of element e = t + 256 i, advanced without a division per element
        int r = t / kp, kk = t - r * kp;
        const int dr = 256 / kp, dk = 256 - dr * kp;
        for (int e = t; e < nrows * kp; e += 256) {
            xs[e] = kk < k ? x[(r0 + r) * ldx + kk] : 0.0f;
            r += dr; kk += dk;
            if (kk >= kp) { kk -= kp; ++r; }
        }
    }
    __syncthreads();
    const int n4 = n >> 2;
    const int per = 256 / n4;                              // rows per pass (n4 <= 256)
    const int c = (t % n4) * 4, rl = t / n4;
    if (rl >= per) return;
    float4 bq = make_float4(0.f, 0.f, 0.f, 0.f);
    if (bias) bq = *reinterpret_cast<const float4*>(bias + c);
    // four rows per thread and trip (rows r, r + per, r + 2 per, r + 3 per): one read of the B quad serves four rows -- with one
    // row per trip the kernel was bound by LDS bandwidth (5 ds_read_b128 per 16 FMAs)
    for (int rb = rl; rb < nrows; rb += 4 * per) {
        float4 v[4];
        const float* xr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            const int r = rb + u * per;
            xr[u] = xs + (r < nrows ? r : rb) * kp;              // (rows past the end: recomputed, never stored)
        }
        for (int kk = 0; kk < kp; kk += 4) {
            const float4 w0 = *reinterpret_cast<const float4*>(&bs[kk * n + c]);
            const float4 w1 = *reinterpret_cast<const float4*>(&bs[(kk + 1) * n + c]);
            const float4 w2 = *reinterpret_cast<const float4*>(&bs[(kk + 2) * n + c]);
            const float4 w3 = *reinterpret_cast<const float4*>(&bs[(kk + 3) * n + c]);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float4 a = *reinterpret_cast<const float4*>(xr[u] + kk);
                v[u].x = fmaf(a.x, w0.x, v[u].x); v[u].y = fmaf(a.x, w0.y, v[u].y); v[u].z = fmaf(a.x, w0.z, v[u].z); v[u].w = fmaf(a.x, w0.w, v[u].w);
                v[u].x = fmaf(a.y, w1.x, v[u].x); v[u].y = fmaf(a.y, w1.y, v[u].y); v[u].z = fmaf(a.y, w1.z, v[u].z); v[u].w = fmaf(a.y, w1.w, v[u].w);
                v[u].x = fmaf(a.z, w2.x, v[u].x); v[u].y = fmaf(a.z, w2.y, v[u].y); v[u].z = fmaf(a.z, w2.z, v[u].z); v[u].w = fmaf(a.z, w2.w, v[u].w);
                v[u].x = fmaf(a.w, w3.x, v[u].x); v[u].y = fmaf(a.w, w3.y, v[u].y); v[u].z = fmaf(a.w, w3.z, v[u].z); v[u].w = fmaf(a.w, w3.w, v[u].w);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = rb + u * per;
            if (r >= nrows) break;
            const int64_t row = r0 + r;
            float4 o = v[u];
            if (residual) {
                const float* rrow = xb_res_row(residual, ldr, gate, row);
                if (rrow) { const float4 rq = *reinterpret_cast<const float4*>(rrow + c); o.x += rq.x; o.y += rq.y; o.z += rq.z; o.w += rq.w; }
            }
            o.x += bq.x; o.y += bq.y; o.z += bq.z; o.w += bq.w;
            if (act) {
                o.x = o.x > 0.0f ? o.x : o.x * slope; o.y = o.y > 0.0f ? o.y : o.y * slope;
                o.z = o.z > 0.0f ? o.z : o.z * slope; o.w = o.w > 0.0f ? o.w : o.w * slope;
            }
            if (gate.y || gate.mask || gate.drop.on) xb_gate4(o, gate, row, c);
            *reinterpret_cast<float4*>(y + row * ldy + c) = o;
        }
    }
}

// y = act(sum_z partial[z] + bias + residual): the epilogue of a split-K gemm_xb2 (fixed order over z)
// (workgroup bx of nb: the single kernel's blockIdx.x / gridDim.x, or a member's share of a grouped grid)
__device__ __forceinline__ void splitk_epilogue_body(const unsigned bx, const unsigned nb, const float* __restrict__ partial, int splits,
                                                     int64_t m, int n, float* __restrict__ y, int64_t ldy,
                                                     const float* __restrict__ bias, const float* __restrict__ residual, int64_t ldr,
                                                     int act, float slope, const XbGate& gate)
{
    const int n4 = n >> 2;
    const int64_t total = m * n4;
    for (int64_t e = (int64_t)bx * 256 + threadIdx.x; e < total; e += (int64_t)nb * 256) {
        const int64_t r = e / n4;
        const int c = (int)(e % n4) * 4;
        float4 v = *reinterpret_cast<const float4*>(partial + r * n + c);
        for (int z = 1; z < splits; ++z) {
            const float4 p = *reinterpret_cast<const float4*>(partial + ((int64_t)z * m + r) * n + c);
            v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
        }
        if (bias) { const float4 bq = *reinterpret_cast<const float4*>(bias + c); v.x += bq.x; v.y += bq.y; v.z += bq.z; v.w += bq.w; }
        if (residual) {
            const float* rrow = xb_res_row(residual, ldr, gate, r);
            if (rrow) {
                const float4 rq = *reinterpret_cast<const float4*>(rrow + c);
                v.x += rq.x; v.y += rq.y; v.z += rq.z; v.w += rq.w;
            }
        }
        if (act) {
            v.x = v.x > 0.0f ? v.x : v.x * slope; v.y = v.y > 0.0f ? v.y : v.y * slope;
            v.z = v.z > 0.0f ? v.z : v.z * slope; v.w = v.w > 0.0f ? v.w : v.w * slope;
        }
        xb_gate4(v, gate, r, c);
        *reinterpret_cast<float4*>(y + r * ldy + c) = v;
    }
}

__global__ __launch_bounds__(256) void splitk_epilogue_kernel(const float* __restrict__ partial, int splits, int64_t m, int n,
                                                               float* __restrict__ y, int64_t ldy, const float* __restrict__ bias,
                                                               const float* __restrict__ residual, int64_t ldr, int act, float slope,
                                                               const XbGate gate)
{
    splitk_epilogue_body(blockIdx.x, gridDim.x, partial, splits, m, n, y, ldy, bias, residual, ldr, act, slope, gate);
}

// the split-K epilogues of a grouped gemm_xb2 launch: member j takes nb workgroups (what it takes alone) and adds its
// partial sums in the single kernel's order
struct SplitkProblem {
    const float* partial; int64_t m; float* y; int64_t ldy; const float* bias; const float* residual; int64_t ldr; XbGate gate;
    int splits, n, act; float slope; unsigned nb;
};
struct SplitkGroup { GroupIndex gi; SplitkProblem p[GROUP_MAX]; };
static_assert(sizeof(SplitkGroup) < 4096, "the group travels in the kernel arguments");
__global__ __launch_bounds__(256) void splitk_epilogue_group_kernel(const SplitkGroup g)
{
    unsigned l;
    const SplitkProblem& p = g.p[group_find(g.gi, l)];
    splitk_epilogue_body(l, p.nb, p.partial, p.splits, p.m, p.n, p.y, p.ldy, p.bias, p.residual, p.ldr, p.act, p.slope, p.gate);
}

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

int64_t colsum_chunk(int64_t m)
{
    int64_t c = ws_ceil_div(m, 768);
    return c < 16 ? 16 : c;                             // <= 768 chunks (three workgroups per CU) of >= 16 rows
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// chunk sums -> out: the wide form for large outputs of few chunks, the grouped form otherwise
bool reduce_partials_wide(const void* partial, int64_t elems, int chunks, const void* out, int n, int64_t ldo)
{
    return elems >= 65536 && chunks <= 64 && elems % 4 == 0 && al16(partial) && al16(out) && (ldo <= n || (n % 4 == 0 && ldo % 4 == 0));
}
void launch_reduce_partials(const float* partial, int64_t elems, int chunks, float* out, hipStream_t st, int n = 0, int64_t ldo = 0)
{
    if (reduce_partials_wide(partial, elems, chunks, out, n, ldo))
        reduce_partials_wide_kernel<<<(unsigned)ws_ceil_div(elems, 1024), 256, 0, st>>>(partial, elems, chunks, out, n, ldo);
    else
        reduce_partials_kernel<<<(unsigned)ws_ceil_div(elems, 32), 256, 0, st>>>(partial, elems, chunks, out, n, ldo);
}

int64_t xty_chunk(int64_t m, int k, int n)
{
    if (m >= 32768) {
        // tall operands: <= 256 chunks, a multiple of BK rows each, at least 512 rows (keeps >= 256 workgroups in
        // flight even when K fits one k-tile)
        int64_t c = ws_ceil_div(m, 256);
        if (c < 512) c = 512;
        return ws_ceil_div(c, BK) * BK;
    }
    // short operands (the deep pyramid levels): one chunk is a serial chain of m / 2 MFMA steps per wave, so the rows are
    // split until the chain (A / chunks) balances the write + re-read of the partial outputs (B * chunks):
    //   A = m/2 steps x 4 tiles x 64 cycles at 2.4 GHz,  B = 2 x 4 k n bytes at ~2 TB/s (measured: scattered partial stores),  chunks = sqrt(A / B),
    // at most 256 workgroups (tiles of 128 x 128 outputs x chunks: one per CU -- beyond that the MFMA pipes are shared and
    // more chunks only add partial traffic; 257..511 workgroups would double the time) and at least 32 rows per chunk.
    const double a_us = (double)m * 0.5 * 4.0 * 64.0 / 2400.0;
    const double b_us = 16.0 * (double)k * (double)n / 4.0e6;
    const int64_t tiles = ws_ceil_div(k, 128) * ws_ceil_div(n, 128);
    int64_t chunks = (int64_t)(__builtin_sqrt(a_us / b_us) + 0.5);
    if (chunks > 256 / tiles) chunks = 256 / tiles;
    if (chunks > m / 32) chunks = m / 32;
    if (chunks < 1) chunks = 1;
    return ws_ceil_div(ws_ceil_div(m, chunks), BK) * BK;
}

constexpr int THIN_K = 64;    // products with k <= this take 64-column tiles (more, lighter workgroups: they are all prologue and epilogue) instead of 128

}  // namespace

extern "C" {
// diagnostic switches (not part of the drop-in surface of include/weasal_hip.h)
int ws_gemm_shallow = 1;     // products with k <= 64 that the MFMA tiles do not take (k % 32 != 0), n % 4 == 0, many rows: 1 = gemm_xb_shallow_kernel, 0 = gemm_xb_kernel
int ws_gemm_staged = 1;     // gemm_xb2 epilogue: 1 = the tile turned through LDS (whole 128-byte row segments per store), 0 = per-lane rows
}

// ---------------------------------------------------------------------------------------------
// Host side.  A product travels as a record -- ws_xb_problem / ws_xty_problem (ws_common.h) -- that every entry, single or
// grouped, fills.  Per family: one validator (its messages carry "member <i>: " in a group), one plan shared with the reporter,
// one launcher per kernel that dispatches the plan onto the template arguments (ws_dispatch.h), one run.
// ---------------------------------------------------------------------------------------------
namespace {

// a failed requirement of a product: the message of the single entries (member < 0), behind "member <i>: " for a group's member i
int product_fail(int member, int code, const char* fmt, ...)
{
    char* buf = ws_errbuf();
    const int off = member >= 0 ? snprintf(buf, 512, "member %d: ", member) : 0;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf + off, 512 - (size_t)off, fmt, ap);
    va_end(ap);
    return code;
}
#define PRODUCT_REQUIRE(member, cond, ...) do { if (!(cond)) return product_fail(member, WS_ERR_INVALID, __VA_ARGS__); } while (0)

// ---- gemm_xb ----------------------------------------------------------------------------------------------------------------
int xb_validate(const ws_xb_problem& q, int member)
{
    PRODUCT_REQUIRE(member, q.m >= 0 && q.k >= 1 && q.n >= 1 && q.ldx >= q.k && q.ldy >= q.n, "bad sizes m=%lld k=%d n=%d", (long long)q.m, q.k, q.n);
    PRODUCT_REQUIRE(member, !q.residual || q.ldr >= q.n, "residual leading dimension too small");
    PRODUCT_REQUIRE(member, q.act == 0 || q.act == 1, "unknown activation %d", q.act);
    PRODUCT_REQUIRE(member, q.drop_p >= 0.0f && q.drop_p < 1.0f, "bad drop probability %g", (double)q.drop_p);
    PRODUCT_REQUIRE(member, !q.res_rows || (q.residual && q.res_rows_ld >= 1 && q.res_nrows >= 0), "gathered residual: NULL residual / bad sizes");
    PRODUCT_REQUIRE(member, !q.gate_y || q.ldg >= q.n, "gate leading dimension too small");
    PRODUCT_REQUIRE(member, !q.mask || q.ldm >= q.n, "mask leading dimension too small");
    PRODUCT_REQUIRE(member, q.m == 0 || (q.x && q.b && q.y), "NULL argument");
    return WS_OK;
}

XbGate xb_problem_gate(const ws_xb_problem& q)
{
    XbGate g{};
    g.y = q.gate_y; g.ld = q.ldg; g.slope = q.gate_slope;
    g.mask = q.mask; g.ldm = q.ldm; g.mscale = q.mask_scale;
    g.drop = ws_drop_args(q.drop_p, q.drop_seed);
    g.dn = q.n;
    g.rrows = q.res_rows; g.rld = q.res_rows_ld; g.rn = q.res_nrows;
    return g;
}

// row stride of the small matrix (b_row_stride < 0: row-major [K, N])
int64_t xb_brs(const ws_xb_problem& q) { return q.b_row_stride < 0 ? q.n : q.b_row_stride; }

// The launch a product takes: every selection rule of the xb entries, shared with the reporter ws_gemm_xb_variant (which
// only reads the pointers' alignment).
enum { XB_NONE = 0, XB_XB2 = 1, XB_SHALLOW = 2, XB_GENERIC = 3 };
struct XbPlan {
    int kind;
    int nt, wn;             // XB_XB2: gemm_xb2_kernel<nt, wn>; XB_GENERIC: gemm_xb_kernel<nt, 32>
    dim3 grid;
    int splits, csplit;     // XB_XB2: split-K layers (splits > 1: sums in scratch, then splitk_epilogue_kernel), chunks per layer
    int staged;             // XB_XB2: ws_gemm_staged
    int vecx, vecb;         // XB_GENERIC: float4 loads of x / b
    int rows;               // XB_SHALLOW: rows per workgroup
    size_t lds;             // XB_SHALLOW: dynamic LDS bytes
};

int xb_plan(const ws_xb_problem& q, XbPlan& p)
{
    p = XbPlan{};
    if (q.m == 0) return WS_OK;
    const int64_t m = q.m, brs = xb_brs(q), bcs = q.b_col_stride;
    const int k = q.k, n = q.n;
    const int vecx = al16(q.x) && (q.ldx % 4 == 0);
    const int vecb = al16(q.b) && (n % 4 == 0);
    const int64_t gx = ws_ceil_div(m, BM);
    WS_REQUIRE(gx < (1ll << 31), "m too large");
    // what the float4 epilogues ask of everything they touch
    const bool epi4 = n % 4 == 0 && al16(q.y) && q.ldy % 4 == 0 && (!q.residual || (al16(q.residual) && q.ldr % 4 == 0)) &&
                      (!q.bias || al16(q.bias)) && (!q.gate_y || (al16(q.gate_y) && q.ldg % 4 == 0)) &&
                      (!q.mask || ((reinterpret_cast<uintptr_t>(q.mask) & 3u) == 0 && q.ldm % 4 == 0));
    if (vecx && k % 32 == 0 && epi4 && (int64_t)(k - 1) * brs + (int64_t)(n - 1) * bcs < (1ll << 29) && 128 * q.ldx < (1ll << 29) &&
        al16(q.b) && (bcs == 1 ? true : (brs == 1 && bcs % 4 == 0))) {
        const int64_t tiles = ws_ceil_div(m, 32);
        int wn = tiles >= 2048 ? 1 : 2;
        if (n <= 32) wn = 1;
        const int nt = wn == 1 ? (n <= 32 ? 1 : (n <= 64 || k <= THIN_K) ? 2 : 4) : (n <= 64 ? 1 : 2);
        const unsigned gx2 = (unsigned)ws_ceil_div(m, 32 * (4 / wn)), gy2 = (unsigned)ws_ceil_div(n, 32 * nt * wn);
        const int nch = k / 32;
        int splits = 1;
        if (q.scratch && (int64_t)gx2 * gy2 < 256 && nch >= 16) {
            splits = (int)ws_ceil_div(768, (int64_t)gx2 * gy2);
            if (splits > nch / 8) splits = nch / 8;
            if (splits > 16) splits = 16;
            if ((int64_t)splits * m * n * 4 > q.scratch_bytes) splits = (int)(q.scratch_bytes / (m * n * 4));
            if (splits < 2) splits = 1;
        }
        const int csplit = (int)ws_ceil_div(nch, splits);
        splits = (int)ws_ceil_div(nch, csplit);
        p.kind = XB_XB2; p.nt = nt; p.wn = wn; p.grid = dim3(gx2, gy2, (unsigned)splits);
        p.splits = splits; p.csplit = csplit; p.staged = ws_gemm_staged;
        return WS_OK;
    }
    WS_REQUIRE(bcs == 1 && brs == n, "a strided small matrix needs k %% 32 == 0, n %% 4 == 0 and 16-byte aligned rows "
                                     "(k=%d n=%d): pass a row-major [K,N] copy for this shape", k, n);
    if (ws_gemm_shallow && k <= 64 && n <= 1024 && (int64_t)k * n <= 8192 && m >= 4096 && al16(q.b) && epi4) {
        // shallow, ragged contraction over many rows: the streaming VALU form (gemm_xb_shallow_kernel)
        const int per = 256 / (n / 4);
        const int kp = (k + 3) & ~3;
        p.kind = XB_SHALLOW;
        p.rows = per * 8;                                               // 8 row passes per workgroup
        p.grid = dim3((unsigned)ws_ceil_div(m, p.rows));
        p.lds = sizeof(float) * ((size_t)kp * n + (size_t)p.rows * kp);
        return WS_OK;
    }
    p.kind = XB_GENERIC; p.vecx = vecx; p.vecb = vecb;
    // measured (tools/gemm_bench.py, M = 400k): for n > 64, shallow K is latency bound and prefers the 64-column
    // tile (more waves per SIMD, L2 serves the X re-read); deep K prefers the 128-column tile (X reuse)
    p.nt = n <= 32 ? 1 : (n <= 64 || k < 128) ? 2 : 4;
    p.grid = dim3((unsigned)gx, n <= 64 ? 1u : (unsigned)ws_ceil_div(n, 32 * p.nt));
    return WS_OK;
}

// the (NT, WN) of gemm_xb2_kernel / gemm_xb2_group_kernel that exist; the index is the bucket of the grouped entry
constexpr int XB2_PAIRS[][2] = {{1, 1}, {2, 1}, {4, 1}, {1, 2}, {2, 2}};
constexpr int XB2_NPAIRS = 5;
constexpr int xb2_pair(int nt, int wn)
{
    for (int i = 0; i < XB2_NPAIRS; ++i)
        if (XB2_PAIRS[i][0] == nt && XB2_PAIRS[i][1] == wn) return i;
    return -1;
}
int xb2_no_instantiation(const XbPlan& p) { return ws_no_instantiation("gemm_xb2_kernel<NT=%d, WN=%d>", p.nt, p.wn); }

int launch_xb2(const ws_xb_problem& q, const XbPlan& p, const XbGate& gate, hipStream_t st)
{
    float* part = p.splits > 1 ? (float*)q.scratch : nullptr;
    bool pruned = false;
    const bool called = dispatch([&](auto nt, auto wn) {
        if constexpr (xb2_pair(nt.value, wn.value) >= 0)
            gemm_xb2_kernel<nt.value, wn.value><<<p.grid, 256, 0, st>>>(q.x, q.m, q.k, q.ldx, q.b, q.n, (int)xb_brs(q), (int)q.b_col_stride, q.y,
                                                                        q.ldy, q.bias, q.residual, q.ldr, q.act, q.slope, p.csplit, part, gate,
                                                                        p.staged);
        else pruned = true;
    }, Pick<1, 2, 4>{p.nt}, Pick<1, 2>{p.wn});
    return called && !pruned ? WS_OK : xb2_no_instantiation(p);
}

// the epilogue of ONE split product (p.splits > 1): it counts with its product's launch (ws_common.h)
void launch_splitk_epilogue(const ws_xb_problem& q, const XbPlan& p, const XbGate& gate, hipStream_t st)
{
    splitk_epilogue_kernel<<<ws_grid(q.m * (q.n / 4), 256), 256, 0, st>>>((const float*)q.scratch, p.splits, q.m, q.n, q.y, q.ldy, q.bias,
                                                                          q.residual, q.ldr, q.act, q.slope, gate);
}

int launch_xb_generic(const ws_xb_problem& q, const XbPlan& p, const XbGate& gate, hipStream_t st)
{
    const bool called = dispatch([&](auto nt) {
        gemm_xb_kernel<nt.value, 32><<<p.grid, 256, 0, st>>>(q.x, q.m, q.k, q.ldx, q.b, q.n, q.n, q.y, q.ldy, p.vecx, p.vecb, q.bias, q.residual,
                                                             q.ldr, q.act, q.slope, gate);
    }, Pick<1, 2, 4>{p.nt});
    return called ? WS_OK : ws_no_instantiation("gemm_xb_kernel<NT=%d, BKX=32>", p.nt);
}

// product q (m > 0) by its plan: ONE counted launch
int xb_launch(const ws_xb_problem& q, const XbPlan& p, hipStream_t st)
{
    const XbGate gate = xb_problem_gate(q);
    int rc = WS_OK;
    if (p.kind == XB_XB2) {
        rc = launch_xb2(q, p, gate, st);
        if (rc == WS_OK && p.splits > 1) launch_splitk_epilogue(q, p, gate, st);
    } else if (p.kind == XB_SHALLOW) {
        gemm_xb_shallow_kernel<<<p.grid, 256, p.lds, st>>>(q.x, q.m, q.k, q.ldx, q.b, q.n, q.y, q.ldy, q.bias, q.residual, q.ldr, q.act, q.slope,
                                                           gate, p.rows);
    } else {
        rc = launch_xb_generic(q, p, gate, st);
    }
    if (rc != WS_OK) return rc;
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int xb_run(const ws_xb_problem& q, void* stream)
{
    int rc = xb_validate(q, -1);
    if (rc != WS_OK || q.m == 0) return rc;
    XbPlan p;
    rc = xb_plan(q, p);
    return rc != WS_OK ? rc : xb_launch(q, p, (hipStream_t)stream);
}

// the record of the plain product y = x b, b row-major [K, N]: the entries add their strides, epilogue and gates
ws_xb_problem xb_problem(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int32_t n, float* y, int64_t ldy,
                         void* scratch = nullptr, int64_t scratch_bytes = 0)
{
    ws_xb_problem q{};
    q.x = x; q.m = m; q.k = k; q.ldx = ldx;
    q.b = b; q.b_row_stride = -1; q.b_col_stride = 1; q.n = n;
    q.y = y; q.ldy = ldy;
    q.scratch = scratch; q.scratch_bytes = scratch_bytes;
    return q;
}
void xb_epilogue(ws_xb_problem& q, const float* bias, const float* residual, int64_t ldr, int32_t act, float slope)
{
    q.bias = bias; q.residual = residual; q.ldr = ldr; q.act = act; q.slope = slope;
}
void xb_strides(ws_xb_problem& q, int64_t b_row_stride, int64_t b_col_stride)
{
    q.b_row_stride = b_row_stride; q.b_col_stride = b_col_stride;
}

// ---- grouped products (ws_common.h) ------------------------------------------------------------------------------------------
// Each member keeps exactly the plan it gets alone from xb_plan / xty_plan -- kind, tile variant, splits, csplit, chunk,
// chunks, reduction form, pitched output -- and its workgroups run the single kernels' bodies on that plan, so every sum
// is added in the order of the single launch: a grouped result is bit-identical to the single one.  Only the number of
// launches changes.
// one call plans at most GROUP_CALL_MAX members on the stack (no allocation on the launch path: the block calls pass 2 .. 4);
// a longer list is handled as consecutive slices of that many, each grouped within itself
constexpr int GROUP_CALL_MAX = 16;
struct IdList {
    int n = 0;
    int v[GROUP_CALL_MAX];
    void push_back(int i) { v[n++] = i; }
    int size() const { return n; }
};
constexpr int64_t GROUP_MEMBER_BLOCKS = 1ll << 27;      // a member with more workgroups runs alone (the linear index stays 32-bit)

// the members of one instantiation, GROUP_MAX at a time (more spill into further launches): f(ids, cnt) -> WS_OK or the error
template <typename F>
int for_each_launch(const IdList& ids, F&& f)
{
    for (int off = 0; off < ids.size(); off += GROUP_MAX) {
        const int rc = f(ids.v + off, ids.size() - off < GROUP_MAX ? ids.size() - off : GROUP_MAX);
        if (rc != WS_OK) return rc;
    }
    return WS_OK;
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

int launch_xb2_group(const ws_xb_problem* q, const XbPlan* plan, const int* ids, int cnt, hipStream_t st)
{
    Xb2Group g{};
    SplitkGroup e{};
    GroupFill gf{g.gi}, ef{e.gi};
    int last_e = -1;
    for (int j = 0; j < cnt; ++j) {
        const ws_xb_problem& a = q[ids[j]];
        const XbPlan& p = plan[ids[j]];
        const XbGate gate = xb_problem_gate(a);
        float* part = p.splits > 1 ? (float*)a.scratch : nullptr;
        g.p[j] = Xb2Problem{a.x, a.m, a.ldx, a.b, a.y, a.ldy, a.bias, a.residual, a.ldr, part, gate, a.k, a.n,
                            (int)xb_brs(a), (int)a.b_col_stride, a.act, p.csplit, p.staged, a.slope, p.grid.x, p.grid.y};
        gf.add(p.grid.x * p.grid.y * p.grid.z);
        if (p.splits > 1) {
            const unsigned nb = (unsigned)ws_grid(a.m * (a.n / 4), 256);
            e.p[ef.n] = SplitkProblem{part, a.m, a.y, a.ldy, a.bias, a.residual, a.ldr, gate, p.splits, a.n, a.act, a.slope, nb};
            ef.add(nb);
            last_e = ids[j];
        }
    }
    const XbPlan& p0 = plan[ids[0]];        // (the bucket's instantiation: xb2_pair)
    bool pruned = false;
    const bool called = dispatch([&](auto nt, auto wn) {
        if constexpr (xb2_pair(nt.value, wn.value) >= 0) gemm_xb2_group_kernel<nt.value, wn.value><<<gf.total, 256, 0, st>>>(g);
        else pruned = true;
    }, Pick<1, 2, 4>{p0.nt}, Pick<1, 2>{p0.wn});
    if (!called || pruned) return xb2_no_instantiation(p0);
    WS_LAUNCH_CHECK();
    if (ef.n == 1) {
        launch_splitk_epilogue(q[last_e], plan[last_e], xb_problem_gate(q[last_e]), st);
        WS_HIP(hipGetLastError());      // (a single split epilogue counts with its product, as in xb_launch: ws_common.h)
    } else if (ef.n > 1) {
        splitk_epilogue_group_kernel<<<ef.total, 256, 0, st>>>(e);
        WS_LAUNCH_CHECK();
    }
    return WS_OK;
}

// ---- gemm_xty -----------------------------------------------------------------------------------------------------------------
// bf16 rows (ws_gemm_xty_bf16) travel in the same record, x and y pointing at 2-byte elements: the row type is the `bf16` beside it
int xty_validate(const ws_xty_problem& q, int member)
{
    PRODUCT_REQUIRE(member, q.m >= 0 && q.k >= 1 && q.n >= 1 && q.ldx >= q.k && q.ldy >= q.n, "bad sizes m=%lld k=%d n=%d", (long long)q.m, q.k, q.n);
    PRODUCT_REQUIRE(member, q.out, "NULL argument");
    PRODUCT_REQUIRE(member, q.ldo == 0 || q.ldo >= q.n, "output pitch smaller than a row");
    PRODUCT_REQUIRE(member, q.m == 0 || (q.x && q.y && q.scratch), "NULL argument");
    return WS_OK;
}

// The launches of a dW reduction: every selection rule of the xty entries, shared with the reporter ws_gemm_xty_variant
// (which only reads the pointers' alignment).  bf16: 2-byte operands (no gemm_xty_kernel fallback).
struct XtyPlan {
    int bf16;
    int lds;                // 0: gemm_xty2_kernel<kt, nt, wk, wn>; 1: gemm_xty_kernel<nt, kt> (32-bit buffer offsets overflow)
    int kt, nt, wk, wn;
    int vecx, vecy;         // gemm_xty_kernel: float4 loads
    int64_t chunk;
    int chunks;
    float* partial;         // out itself (one chunk, flat) or the scratch
    int reduce;             // 0: none, 1: reduce_partials_kernel, 2: reduce_partials_wide_kernel
    bool pitched;           // ldo > n: `out` is a column block of a wider matrix (row pitch ldo): the chunk sums go through the scratch
    dim3 grid;              //   and the reduction writes the pitched rows (also for one chunk, where it is the copy a caller would make)
};

int xty_plan(const ws_xty_problem& q, bool bf16, XtyPlan& p)
{
    p = XtyPlan{};
    p.bf16 = bf16;
    p.pitched = q.ldo > q.n;
    if (q.m == 0) return WS_OK;
    const int k = q.k, n = q.n;
    p.chunk = xty_chunk(q.m, k, n);
    p.chunks = (int)ws_ceil_div(q.m, p.chunk);
    const int64_t span = p.chunk * (q.ldx > q.ldy ? q.ldx : q.ldy);
    if (bf16) WS_REQUIRE(span * 2 < (1ll << 31), "operand exceeds the 32-bit buffer offsets");
    p.partial = (p.chunks == 1 && !p.pitched) ? q.out : (float*)q.scratch;
    p.lds = !bf16 && span * 4 >= (1ll << 31);
    if (!p.lds) {
        // per-wave tile (32 KT) x (32 NT); waves WK x WN over the output, the rest split the rows
        const bool a2x = bf16 ? (reinterpret_cast<uintptr_t>(q.x) & 3u) == 0 && q.ldx % 2 == 0 && k % 2 == 0
                              : (reinterpret_cast<uintptr_t>(q.x) & 7u) == 0 && q.ldx % 2 == 0;
        const bool a2y = bf16 ? (reinterpret_cast<uintptr_t>(q.y) & 3u) == 0 && q.ldy % 2 == 0 && n % 2 == 0
                              : (reinterpret_cast<uintptr_t>(q.y) & 7u) == 0 && q.ldy % 2 == 0;
        p.kt = (k > 32 && a2x) ? 2 : 1;
        p.nt = (n > 32 && a2y) ? 2 : 1;
        p.wk = k > 32 * p.kt ? 2 : 1;
        p.wn = (n > 32 * p.nt && p.wk == 1) || (n > 32 * p.nt && k > 32 * p.kt) ? 2 : 1;
        p.grid = dim3(p.chunks, (unsigned)ws_ceil_div(k, 32 * p.kt * p.wk), (unsigned)ws_ceil_div(n, 32 * p.nt * p.wn));
    } else {
        p.vecx = al16(q.x) && (q.ldx % 4 == 0);
        p.vecy = al16(q.y) && (q.ldy % 4 == 0);
        p.kt = k <= 32 ? 1 : (k <= 64 ? 2 : 4);
        p.nt = n <= 32 ? 1 : (n <= 64 ? 2 : 4);
        p.grid = dim3(p.chunks, (unsigned)ws_ceil_div(k, 32 * p.kt), (unsigned)ws_ceil_div(n, 32 * p.nt));
    }
    if (p.chunks > 1 || p.pitched)
        p.reduce = reduce_partials_wide(p.partial, (int64_t)k * n, p.chunks, q.out, n, p.pitched ? q.ldo : 0) ? 2 : 1;
    return WS_OK;
}

int xty2_no_instantiation(const XtyPlan& p)
{
    return ws_no_instantiation("gemm_xty2_kernel<KT=%d, NT=%d, WK=%d, WN=%d> bf16=%d", p.kt, p.nt, p.wk, p.wn, p.bf16);
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

// the product launch of plan p: counted
int xty_product_launch(const ws_xty_problem& q, const XtyPlan& p, hipStream_t st)
{
    const int rc = p.lds ? launch_xty_lds(q, p, st) : launch_xty2(q, p, st);
    if (rc != WS_OK) return rc;
    WS_LAUNCH_CHECK();
    return WS_OK;
}
// the chunk sums of plan p (p.reduce != 0): counted
int xty_reduce_launch(const ws_xty_problem& q, const XtyPlan& p, hipStream_t st)
{
    launch_reduce_partials(p.partial, (int64_t)q.k * q.n, p.chunks, q.out, st, q.n, p.pitched ? q.ldo : 0);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int xty_run(const ws_xty_problem& q, bool bf16, void* stream)
{
    int rc = xty_validate(q, -1);
    if (rc != WS_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (q.m == 0) {
        if (q.ldo > q.n) WS_HIP(hipMemset2DAsync(q.out, sizeof(float) * (size_t)q.ldo, 0, sizeof(float) * (size_t)q.n, (size_t)q.k, st));
        else WS_HIP(hipMemsetAsync(q.out, 0, sizeof(float) * (size_t)q.k * q.n, st));
        return WS_OK;
    }
    XtyPlan p;
    rc = xty_plan(q, bf16, p);
    if (rc == WS_OK) rc = xty_product_launch(q, p, st);
    if (rc == WS_OK && p.reduce) rc = xty_reduce_launch(q, p, st);
    return rc;
}

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
    if (!called) return xty2_no_instantiation(p0);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int launch_reduce_group(const ws_xty_problem* q, const XtyPlan* plan, const int* ids, int cnt, hipStream_t st)
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
    WS_LAUNCH_CHECK();
    return WS_OK;
}

const char* reduce_name(int r)
{
    return r == 2 ? "reduce_partials_wide_kernel" : (r == 1 ? "reduce_partials_kernel" : "none");
}

}  // namespace

extern "C" {

int64_t ws_gemm_xb_scratch_bytes(int64_t m, int32_t k, int32_t n)
{
    // room for up to 16 split-K partial outputs; only short, deep products use it
    if (m <= 0 || m >= 32768 || k < 512) return 0;
    return 16 * m * (int64_t)n * (int64_t)sizeof(float);
}

int ws_gemm_xb(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int32_t n, float* y, int64_t ldy,
               void* stream)
{
    return xb_run(xb_problem(x, m, k, ldx, b, n, y, ldy), stream);
}

int ws_gemm_xb_epilogue(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int32_t n,
                        const float* bias, const float* residual, int64_t ldr, int32_t act, float slope,
                        float* y, int64_t ldy, void* stream)
{
    ws_xb_problem q = xb_problem(x, m, k, ldx, b, n, y, ldy);
    xb_epilogue(q, bias, residual, ldr, act, slope);
    return xb_run(q, stream);
}

int ws_gemm_xb_epilogue_splitk(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int32_t n,
                               const float* bias, const float* residual, int64_t ldr, int32_t act, float slope,
                               float* y, int64_t ldy, void* scratch, int64_t scratch_bytes, void* stream)
{
    ws_xb_problem q = xb_problem(x, m, k, ldx, b, n, y, ldy, scratch, scratch_bytes);
    xb_epilogue(q, bias, residual, ldr, act, slope);
    return xb_run(q, stream);
}

int ws_gemm_xb_epilogue_strided(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int64_t b_row_stride,
                                int64_t b_col_stride, int32_t n, const float* bias, const float* residual, int64_t ldr,
                                int32_t act, float slope, float* y, int64_t ldy, void* scratch, int64_t scratch_bytes,
                                void* stream)
{
    ws_xb_problem q = xb_problem(x, m, k, ldx, b, n, y, ldy, scratch, scratch_bytes);
    xb_strides(q, b_row_stride, b_col_stride);
    xb_epilogue(q, bias, residual, ldr, act, slope);
    return xb_run(q, stream);
}

int ws_gemm_xb_gated_strided(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int64_t b_row_stride,
                             int64_t b_col_stride, int32_t n, const float* bias, const float* residual, int64_t ldr,
                             int32_t act, float slope, const float* gate_y, int64_t ldg, float gate_slope, const uint8_t* mask,
                             int64_t ldm, float mask_scale, float* y, int64_t ldy, void* scratch, int64_t scratch_bytes,
                             void* stream)
{
    ws_xb_problem q = xb_problem(x, m, k, ldx, b, n, y, ldy, scratch, scratch_bytes);
    xb_strides(q, b_row_stride, b_col_stride);
    xb_epilogue(q, bias, residual, ldr, act, slope);
    q.gate_y = gate_y; q.ldg = ldg; q.gate_slope = gate_slope;
    q.mask = mask; q.ldm = ldm; q.mask_scale = mask_scale;
    return xb_run(q, stream);
}

int ws_gemm_xb_dropout_strided(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int64_t b_row_stride,
                               int64_t b_col_stride, int32_t n, const float* bias, const float* residual, int64_t ldr,
                               int32_t act, float slope, float drop_p, uint64_t drop_seed, float* y, int64_t ldy, void* scratch,
                               int64_t scratch_bytes, void* stream)
{
    ws_xb_problem q = xb_problem(x, m, k, ldx, b, n, y, ldy, scratch, scratch_bytes);
    xb_strides(q, b_row_stride, b_col_stride);
    xb_epilogue(q, bias, residual, ldr, act, slope);
    q.drop_p = drop_p; q.drop_seed = drop_seed;
    return xb_run(q, stream);
}

int ws_gemm_xb_gate_dropout(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int32_t n, const float* gate_y,
                            int64_t ldg, float gate_slope, float drop_p, uint64_t drop_seed, float* y, int64_t ldy, void* scratch,
                            int64_t scratch_bytes, void* stream)
{
    ws_xb_problem q = xb_problem(x, m, k, ldx, b, n, y, ldy, scratch, scratch_bytes);
    q.gate_y = gate_y; q.ldg = ldg; q.gate_slope = gate_slope;
    q.drop_p = drop_p; q.drop_seed = drop_seed;
    return xb_run(q, stream);
}

// private to the library (ws_common.h): the strided product with the whole epilogue menu -- dropout (drop_p > 0) and / or a
// gathered residual (res_rows != NULL: row r adds residual[res_rows[r * res_rows_ld]], indices outside [0, res_nrows) add nothing)
int ws_priv_gemm_xb_ex(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int64_t b_row_stride, int64_t b_col_stride,
                       int32_t n, const float* bias, const float* residual, int64_t ldr, const int64_t* res_rows, int64_t res_rows_ld,
                       int64_t res_nrows, int32_t act, float slope, float drop_p, uint64_t drop_seed, float* y, int64_t ldy,
                       void* scratch, int64_t scratch_bytes, void* stream)
{
    ws_xb_problem q = xb_problem(x, m, k, ldx, b, n, y, ldy, scratch, scratch_bytes);
    xb_strides(q, b_row_stride, b_col_stride);
    xb_epilogue(q, bias, residual, ldr, act, slope);
    q.res_rows = res_rows; q.res_rows_ld = res_rows_ld; q.res_nrows = res_nrows;
    q.drop_p = drop_p; q.drop_seed = drop_seed;
    return xb_run(q, stream);
}

// private to the library (ws_common.h).  Members whose plan is not gemm_xb2 (the shallow and generic forms) run alone, as do
// members alone in their instantiation; m == 0 does what the single entry does (nothing); more than GROUP_MAX members of one
// instantiation spill into a second launch.
int ws_priv_gemm_xb_group(const ws_xb_problem* q, int32_t count, void* stream)
{
    WS_REQUIRE(count >= 0 && (q || count == 0), "bad group");
    for (; count > GROUP_CALL_MAX; q += GROUP_CALL_MAX, count -= GROUP_CALL_MAX) {
        const int rc = ws_priv_gemm_xb_group(q, GROUP_CALL_MAX, stream);
        if (rc != WS_OK) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    XbPlan plan[GROUP_CALL_MAX];
    IdList bucket[XB2_NPAIRS];
    for (int i = 0; i < count; ++i) {
        int rc = xb_validate(q[i], i);
        if (rc != WS_OK) return rc;
        if (q[i].m == 0) continue;
        const XbPlan& p = plan[i];
        rc = xb_plan(q[i], plan[i]);
        if (rc != WS_OK) return rc;
        if (p.kind != XB_XB2 || (int64_t)p.grid.x * p.grid.y * p.grid.z >= GROUP_MEMBER_BLOCKS) {
            rc = xb_launch(q[i], p, st);
            if (rc != WS_OK) return rc;
            continue;
        }
        if (xb2_pair(p.nt, p.wn) < 0) return xb2_no_instantiation(p);
        bucket[xb2_pair(p.nt, p.wn)].push_back(i);
    }
    for (const IdList& ids : bucket) {
        const int rc = for_each_launch(ids, [&](const int* id, int cnt) {
            return cnt == 1 ? xb_launch(q[id[0]], plan[id[0]], st) : launch_xb2_group(q, plan, id, cnt, st);
        });
        if (rc != WS_OK) return rc;
    }
    return WS_OK;
}

int64_t ws_act_bwd_colsum_scratch_bytes(int64_t m, int32_t n)
{
    return ws_ceil_div(m > 0 ? m : 1, colsum_chunk(m)) * (int64_t)n * (int64_t)sizeof(float);
}

// The launches of act_bwd_colsum_impl (m > 0), shared with the reporter ws_act_bwd_colsum_variant
struct ColsumPlan {
    int v;                  // act_bwd_colsum_kernel<v>: 4 = float4 columns, 1 = any n
    int64_t chunk;
    int chunks;
    float* partial;         // NULL (no column sums), colsum itself (one chunk) or the scratch
    int reduce;             // 1: reduce_partials_kernel adds the chunks
    dim3 grid;
};

static ColsumPlan colsum_plan(const void* dy, int64_t m, int32_t n, int64_t lddy, const void* y, int64_t ldy, const void* dz,
                              int64_t lddz, float* colsum, void* scratch)
{
    ColsumPlan p{};
    p.chunk = colsum_chunk(m);
    p.chunks = (int)ws_ceil_div(m, p.chunk);
    p.partial = colsum ? (p.chunks == 1 ? colsum : (float*)scratch) : nullptr;
    p.reduce = colsum && p.chunks > 1;
    const bool vec = n % 4 == 0 && al16(dy) && lddy % 4 == 0 && (!y || (al16(y) && ldy % 4 == 0 && al16(dz) && lddz % 4 == 0));
    p.v = vec ? 4 : 1;
    p.grid = dim3(p.chunks, (unsigned)ws_ceil_div(ws_ceil_div(n, p.v), 256));
    return p;
}

static int act_bwd_colsum_impl(const float* dy, int64_t m, int32_t n, int64_t lddy, const float* y, int64_t ldy, float slope,
                               float* dz, int64_t lddz, float* colsum, void* scratch, void* stream, WsDrop drop)
{
    WS_REQUIRE(m >= 0 && n >= 1 && lddy >= n, "bad sizes m=%lld n=%d", (long long)m, n);
    WS_REQUIRE(!y || (dz && ldy >= n && lddz >= n), "activation backward needs y and dz");
    WS_REQUIRE(!colsum || scratch, "column sums need scratch");
    hipStream_t st = (hipStream_t)stream;
    if (m == 0) {
        if (colsum) WS_HIP(hipMemsetAsync(colsum, 0, sizeof(float) * (size_t)n, st));
        return WS_OK;
    }
    WS_REQUIRE(dy && (y || colsum), "NULL argument");
    const ColsumPlan p = colsum_plan(dy, m, n, lddy, y, ldy, dz, lddz, colsum, scratch);
    const bool called = dispatch([&](auto v) {
        act_bwd_colsum_kernel<v.value><<<p.grid, 256, 0, st>>>(dy, y, m, n, lddy, ldy, slope, dz, lddz, p.partial, p.chunk, drop);
    }, Pick<1, 4>{p.v});
    if (!called) return ws_no_instantiation("act_bwd_colsum_kernel<V=%d>", p.v);
    WS_LAUNCH_CHECK();
    if (p.reduce) {
        reduce_partials_kernel<<<(unsigned)ws_ceil_div(n, 32), 256, 0, st>>>(p.partial, n, p.chunks, colsum);
        WS_LAUNCH_CHECK();
    }
    return WS_OK;
}

int ws_act_bwd_colsum(const float* dy, int64_t m, int32_t n, int64_t lddy, const float* y, int64_t ldy, float slope,
                      float* dz, int64_t lddz, float* colsum, void* scratch, void* stream)
{
    return act_bwd_colsum_impl(dy, m, n, lddy, y, ldy, slope, dz, lddz, colsum, scratch, stream, WsDrop{});
}

int ws_act_bwd_colsum_dropout(const float* dy, int64_t m, int32_t n, int64_t lddy, const float* y, int64_t ldy, float slope,
                              float drop_p, uint64_t drop_seed, float* dz, int64_t lddz, float* colsum, void* scratch, void* stream)
{
    WS_REQUIRE(drop_p >= 0.0f && drop_p < 1.0f, "bad drop probability %g", (double)drop_p);
    WS_REQUIRE(y && dz, "the dropout form writes dz (it needs y and dz)");
    return act_bwd_colsum_impl(dy, m, n, lddy, y, ldy, slope, dz, lddz, colsum, scratch, stream, ws_drop_args(drop_p, drop_seed));
}

int64_t ws_gemm_xty_scratch_bytes(int64_t m, int32_t k, int32_t n)
{
    // (xty_chunk(0, ..) is 0: size an empty operand as one row, like ws_act_bwd_colsum_scratch_bytes)
    const int64_t rows = m > 0 ? m : 1;
    return ws_ceil_div(rows, xty_chunk(rows, k, n)) * (int64_t)k * n * (int64_t)sizeof(float);
}

int ws_gemm_xty(const float* x, int64_t m, int32_t k, int64_t ldx, const float* y, int32_t n, int64_t ldy,
                float* out, void* scratch, void* stream)
{
    return xty_run(ws_xty_problem{x, m, k, ldx, y, n, ldy, out, 0, scratch, 0}, false, stream);
}

// dW = X^T dY with bf16 rows (BASELINE config 5): the LDS-free reduction with 2-byte operand loads; no pitched form.
// Requirements: k, n even or <= 32 handled by the one-column form; every shape of the bf16 path qualifies.
int ws_gemm_xty_bf16(const uint16_t* x, int64_t m, int32_t k, int64_t ldx, const uint16_t* y, int32_t n, int64_t ldy,
                     float* out, void* scratch, void* stream)
{
    return xty_run(ws_xty_problem{(const float*)x, m, k, ldx, (const float*)y, n, ldy, out, 0, scratch, 0}, true, stream);
}

// private to the library (ws_common.h): dW written as a column block of a wider matrix (row pitch ldo >= n)
int ws_priv_gemm_xty_pitched(const float* x, int64_t m, int32_t k, int64_t ldx, const float* y, int32_t n, int64_t ldy, float* out,
                             int64_t ldo, void* scratch, void* stream)
{
    WS_REQUIRE(ldo >= n, "output pitch smaller than a row");      // (this entry has no ldo = 0: the record's flat form)
    return xty_run(ws_xty_problem{x, m, k, ldx, y, n, ldy, out, ldo, scratch, 0}, false, stream);
}

// private to the library (ws_common.h).  Members in the 32-bit-overflow form (gemm_xty_kernel) run alone, reduction
// included; m == 0 clears the output like the single entry.  The others launch their products grouped by instantiation
// (alone when nobody shares it; more than GROUP_MAX spill into a second launch), then the chunk sums of all of them are
// added by grouped reduction launches of up to GROUP_MAX members.
int ws_priv_gemm_xty_group(const ws_xty_problem* q, int32_t count, void* stream)
{
    WS_REQUIRE(count >= 0 && (q || count == 0), "bad group");
    for (; count > GROUP_CALL_MAX; q += GROUP_CALL_MAX, count -= GROUP_CALL_MAX) {
        const int rc = ws_priv_gemm_xty_group(q, GROUP_CALL_MAX, stream);
        if (rc != WS_OK) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    XtyPlan plan[GROUP_CALL_MAX];
    IdList bucket[16], red;
    for (int i = 0; i < count; ++i) {
        const ws_xty_problem& a = q[i];
        int rc = xty_validate(a, i);
        if (rc != WS_OK) return rc;
        if (a.m > 0 && a.scratch_bytes < ws_gemm_xty_scratch_bytes(a.m, a.k, a.n))
            return product_fail(i, WS_ERR_CAPACITY, "scratch too small: %lld < %lld bytes", (long long)a.scratch_bytes,
                                (long long)ws_gemm_xty_scratch_bytes(a.m, a.k, a.n));
        const XtyPlan& p = plan[i];
        rc = xty_plan(a, false, plan[i]);
        if (rc != WS_OK) return rc;
        if (a.m == 0 || p.lds || (int64_t)p.grid.x * p.grid.y * p.grid.z >= GROUP_MEMBER_BLOCKS) {
            rc = xty_run(a, false, stream);
            if (rc != WS_OK) return rc;
            continue;
        }
        bucket[(((p.kt - 1) * 2 + (p.nt - 1)) * 2 + (p.wk - 1)) * 2 + (p.wn - 1)].push_back(i);
        if (p.reduce) red.push_back(i);
    }
    for (const IdList& ids : bucket) {
        const int rc = for_each_launch(ids, [&](const int* id, int cnt) {
            return cnt == 1 ? xty_product_launch(q[id[0]], plan[id[0]], st) : launch_xty2_group(q, plan, id, cnt, st);
        });
        if (rc != WS_OK) return rc;
    }
    return for_each_launch(red, [&](const int* id, int cnt) {
        return cnt == 1 ? xty_reduce_launch(q[id[0]], plan[id[0]], st) : launch_reduce_group(q, plan, id, cnt, st);
    });
}

// ---------------------------------------------------------------------------------------------
// Reporters: the launches the entries above make for these arguments (the same validators and plan functions; pointers are
// only tested for NULL and alignment, nothing is read or launched).  Form: "kernel<template arguments> key=value ...".
// ---------------------------------------------------------------------------------------------
// ws_gemm_xb* / ws_priv_gemm_xb_ex: b_row_stride < 0 = row-major [K, N] (the non-strided entries); gate_y / mask as in
// ws_gemm_xb_gated_strided (dropout and the gathered residual do not change the launch)
int ws_gemm_xb_variant(const float* x, int64_t m, int32_t k, int64_t ldx, const float* b, int64_t b_row_stride, int64_t b_col_stride,
                       int32_t n, const float* bias, const float* residual, int64_t ldr, const float* gate_y, int64_t ldg,
                       const uint8_t* mask, int64_t ldm, const float* y, int64_t ldy, const void* scratch, int64_t scratch_bytes,
                       char* out, int32_t cap)
{
    WS_REQUIRE(out && cap > 0, "bad argument");
    ws_xb_problem q = xb_problem(x, m, k, ldx, b, n, const_cast<float*>(y), ldy, const_cast<void*>(scratch), scratch_bytes);
    xb_strides(q, b_row_stride, b_col_stride);
    q.bias = bias; q.residual = residual; q.ldr = ldr;
    q.gate_y = gate_y; q.ldg = ldg; q.mask = mask; q.ldm = ldm;
    XbPlan p;
    int rc = xb_validate(q, -1);
    if (rc == WS_OK) rc = xb_plan(q, p);
    if (rc != WS_OK) return rc;
    if (p.kind == XB_NONE)
        snprintf(out, (size_t)cap, "none (m == 0)");
    else if (p.kind == XB_XB2)
        snprintf(out, (size_t)cap, "gemm_xb2_kernel<NT=%d, WN=%d> b=%s epilogue=%s splits=%d csplit=%d%s", p.nt, p.wn,
                 xb_brs(q) == 1 ? "transposed" : "rows", p.staged ? "staged" : "lanes", p.splits, p.csplit,
                 p.splits > 1 ? " + splitk_epilogue_kernel" : "");
    else if (p.kind == XB_SHALLOW)
        snprintf(out, (size_t)cap, "gemm_xb_shallow_kernel rows=%d", p.rows);
    else
        snprintf(out, (size_t)cap, "gemm_xb_kernel<NT=%d, BKX=32> vecx=%d vecb=%d", p.nt, p.vecx, p.vecb);
    return WS_OK;
}

// ws_gemm_xty (ldo = 0), ws_priv_gemm_xty_pitched (ldo >= n) and, rows_bf16 = 1, ws_gemm_xty_bf16 (uint16_t rows, ldo = 0)
int ws_gemm_xty_variant(const void* x, int64_t m, int32_t k, int64_t ldx, const void* y, int32_t n, int64_t ldy, float* out_m,
                        int64_t ldo, void* scratch, int32_t rows_bf16, char* out, int32_t cap)
{
    WS_REQUIRE(out && cap > 0, "bad argument");
    WS_REQUIRE(!rows_bf16 || ldo == 0, "the bf16 reduction has no pitched form");
    const ws_xty_problem q{(const float*)x, m, k, ldx, (const float*)y, n, ldy, out_m, ldo, scratch, 0};
    XtyPlan p;
    int rc = xty_validate(q, -1);
    if (rc == WS_OK) rc = xty_plan(q, rows_bf16 != 0, p);
    if (rc != WS_OK) return rc;
    const char* form = p.pitched ? "pitched" : "flat";
    if (m == 0)
        snprintf(out, (size_t)cap, "memset (m == 0) out=%s", form);
    else if (!p.lds)
        snprintf(out, (size_t)cap, "gemm_xty2_kernel<KT=%d, NT=%d, WK=%d, WN=%d, TI=%s> chunk=%lld chunks=%d reduce=%s out=%s", p.kt, p.nt,
                 p.wk, p.wn, rows_bf16 ? "bf16" : "float", (long long)p.chunk, p.chunks, reduce_name(p.reduce), form);
    else
        snprintf(out, (size_t)cap, "gemm_xty_kernel<NT=%d, KT=%d> vecx=%d vecy=%d chunk=%lld chunks=%d reduce=%s out=%s", p.nt, p.kt,
                 p.vecx, p.vecy, (long long)p.chunk, p.chunks, reduce_name(p.reduce), form);
    return WS_OK;
}

// ws_act_bwd_colsum / ws_act_bwd_colsum_dropout (the dropout form launches the same kernels)
int ws_act_bwd_colsum_variant(const float* dy, int64_t m, int32_t n, int64_t lddy, const float* y, int64_t ldy, const float* dz,
                              int64_t lddz, float* colsum, void* scratch, char* out, int32_t cap)
{
    WS_REQUIRE(out && cap > 0, "bad argument");
    WS_REQUIRE(m >= 0 && n >= 1 && lddy >= n, "bad sizes m=%lld n=%d", (long long)m, n);
    if (m == 0) {
        snprintf(out, (size_t)cap, "%s (m == 0)", colsum ? "memset" : "none");
        return WS_OK;
    }
    const ColsumPlan p = colsum_plan(dy, m, n, lddy, y, ldy, dz, lddz, colsum, scratch);
    snprintf(out, (size_t)cap, "act_bwd_colsum_kernel<V=%d> chunk=%lld chunks=%d reduce=%s", p.v, (long long)p.chunk, p.chunks,
             reduce_name(p.reduce));
    return WS_OK;
}

}  // extern "C"
