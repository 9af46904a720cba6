// weasal_amd/csrc/gemm_xb.hip -- the kernels of Y[M,N] = X[M,K] * B[K,N] (forward and dX of the dense products) and their
// launchers: gemm_xb_kernel, gemm_xb2_kernel and its grouped form, gemm_xb_shallow_kernel, the split-K epilogues.  Which of
// them a product takes is gemm.hip's xb_plan; this unit turns a problem record and its plan into kernel arguments.
// The f32-input MFMA and its lane maps: gemm.hip's header.
#include "gemm_device.h"

namespace {

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

// grouped form (GroupIndex, gemm_device.h): the problems by value, each with its own grid
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

// the gates of a problem record as the kernels take them
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

}  // namespace

namespace gemm {

int launch_xb2(const ws_xb_problem& q, const XbPlan& p, hipStream_t st)
{
    const XbGate gate = xb_problem_gate(q);
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
void launch_splitk_epilogue(const ws_xb_problem& q, const XbPlan& p, hipStream_t st)
{
    splitk_epilogue_kernel<<<ws_grid(q.m * (q.n / 4), 256), 256, 0, st>>>((const float*)q.scratch, p.splits, q.m, q.n, q.y, q.ldy, q.bias,
                                                                          q.residual, q.ldr, q.act, q.slope, xb_problem_gate(q));
}

void launch_xb_shallow(const ws_xb_problem& q, const XbPlan& p, hipStream_t st)
{
    gemm_xb_shallow_kernel<<<p.grid, 256, p.lds, st>>>(q.x, q.m, q.k, q.ldx, q.b, q.n, q.y, q.ldy, q.bias, q.residual, q.ldr, q.act, q.slope,
                                                       xb_problem_gate(q), p.rows);
}

int launch_xb_generic(const ws_xb_problem& q, const XbPlan& p, hipStream_t st)
{
    const XbGate gate = xb_problem_gate(q);
    const bool called = dispatch([&](auto nt) {
        gemm_xb_kernel<nt.value, 32><<<p.grid, 256, 0, st>>>(q.x, q.m, q.k, q.ldx, q.b, q.n, q.n, q.y, q.ldy, p.vecx, p.vecb, q.bias, q.residual,
                                                             q.ldr, q.act, q.slope, gate);
    }, Pick<1, 2, 4>{p.nt});
    return called ? WS_OK : ws_no_instantiation("gemm_xb_kernel<NT=%d, BKX=32>", p.nt);
}

// members ids[0 .. cnt) of one instantiation (gemm.hip's bucket) behind one grid, then their split-K epilogues.  This function
// makes several counted launches -- the group kernel, then one epilogue (counted with the products, ws_common.h) or the grouped
// epilogue (one more) -- so it passes the launch checks itself, between them, instead of leaving one to the entry.
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
        launch_splitk_epilogue(q[last_e], plan[last_e], st);
        WS_HIP(hipGetLastError());      // (a single split epilogue counts with its product, as in gemm.hip's xb_launch: ws_common.h)
    } else if (ef.n > 1) {
        splitk_epilogue_group_kernel<<<ef.total, 256, 0, st>>>(e);
        WS_LAUNCH_CHECK();
    }
    return WS_OK;
}

}  // namespace gemm
