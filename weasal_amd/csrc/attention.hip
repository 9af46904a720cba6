// weasal_amd/csrc/attention.hip -- the per-sphere dense attention of the weak-label network KPFCNN_mprm
// (models/blocks.py:758-1011) on the f32-input matrix core, forward and backward.
//
// SPATIAL FORM (spatial_att, blocks.py:788-821): per input sphere  att = softmax(Q K^T) V  (no 1/sqrt(d) scale),
// xn = att / n_sphere;  Q, K [N, dq], V [N, dv], all spheres stacked, one launch for all of them.  The reference (and a
// torch.matmul loop) writes the [n, n] energies and their softmax per sphere to memory, forward and again for autograd;
// here no [n, n] tensor exists:
//   forward   a workgroup owns 64 query rows (16 per wave) and a slice of 64 / 128 columns of dv (grid.y slices, each
//             recomputes its 64 x 64 score tile: dq <= 64 << dv).  Key tiles of 64 stream through LDS (K rows and the V
//             slice); a running row maximum m and row sum l are kept, the accumulator is rescaled by exp(m_old - m_new)
//             when the maximum rises; the probabilities go through a per-wave LDS tile, which turns the MFMA D layout
//             into an A operand.  Key columns past the sphere's end are -inf, query rows past it are not stored, tiles
//             never straddle two spheres, an empty sphere has no tile.  Epilogue: att = acc / l, xn = att / n and, when
//             a backward pass will follow, the row log-sum-exp L = m + log l.
//   backward  recomputes P = exp(S - L):
//             1. sphere_att_pre_kernel   dO = d_att + d_xn / n,  D = rowsum(dO o att)
//             2. sphere_att_dqk_kernel<0>   query tiles:  dQ = (P o (dO V^T - D)) K
//             3. sphere_att_pv_kernel<1>    key tiles:    dV = P^T dO          (sliced over dv like the forward)
//             4. sphere_att_dqk_kernel<1>   key tiles:    dK = dS^T Q
//             dO V^T is formed in both 2 and 4 (2 n^2 dv more flops per sphere): the price of no atomics and no [n, n]
//             scratch.  Every sum has a fixed order: run-to-run bit-identical.
// Widths: dq % 8 == 0, dq <= 64, dv % 64 == 0, dv <= 512.  The multiple of 8 is a policy, not a limit of the kernels: the own-row
// operand and the staged rows are zero-padded to 4 NST columns, so any dq % 4 == 0 would run; dq = 12 has to be refused, and
// 8, 32, 64 are the widths that exist.
// expf / logf, not the fast forms: the network tests hold this path to 1e-4 of the reference.
// Sphere offsets travel BY VALUE in the kernel arguments (up to 64 spheres): no upload, no read-back.
//
// CHANNEL FORM (channel_att, blocks.py:853-882; ele_att, blocks.py:984-1011): per sphere E = X1^T X2 [c, c] (contraction
// over the sphere's rows), A = softmax_rows(t(E)), out = Val A;  t(E) = rowmax(E) - E (channel_att) or E (ele_att).
// The two products are the grouped dense products of gemm.hip with one problem per sphere (ws_priv_gemm_xty_group /
// ws_priv_gemm_xb_group); new here is the row softmax of all [B c, c] rows (one launch) and its backward.
//   backward  dA_b = Val_b^T dOut_b;  softmax backward dT = A o (dA - rowsum(dA o A));  dE = dT (plain) or -dT
//             (max-minus);  dVal = dOut A_b^T,  dX1 = X2 dE^T,  dX2 = X1 dE: 3 B products behind grouped launches.
//             In the max-minus form torch also sends sum_j dT_ij through the row maximum; that sum is zero for a softmax
//             up to rounding (dT = A o (dA - <dA, A>), sum_j A_ij = 1), so it is not replayed.
//             The transposed operands come from the b_row_stride / b_col_stride of ws_xb_problem where the MFMA product
//             takes them (c % 32 == 0); for other widths the softmax backward writes A^T and dE^T beside dE.
#include "ws_common.h"
#include "ws_dispatch.h"
#include <math.h>

namespace {

typedef float f32x4v __attribute__((ext_vector_type(4)));

constexpr int AT_MAX_SPHERES = 64;     // WS_ATT_MAX_SPHERES
constexpr int AT_TQ = 64;              // rows per tile (own rows and streamed rows)
constexpr int AT_YP = 68;              // pitch of the staged [64, dq] rows and of the per-wave P tile: 4 i + kk hits 64 banks
constexpr int AT_DVC = 128;            // dv columns per staged chunk of the dqk kernels (pitch 132: same bank rule)

struct AttSpheres {
    int32_t count;
    int32_t row0[AT_MAX_SPHERES + 1];  // first stacked row of every sphere, row0[count] = N
    int32_t tile0[AT_MAX_SPHERES + 1]; // first 64-row tile of every sphere
};

__device__ __forceinline__ void lds_order()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// sphere and tile of this workgroup
__device__ __forceinline__ void att_tile(const AttSpheres& sp, int& base, int& n, int& tile)
{
    int s = 0;
    while (s + 1 < sp.count && (int)blockIdx.x >= sp.tile0[s + 1]) ++s;
    base = sp.row0[s];
    n = sp.row0[s + 1] - base;
    tile = blockIdx.x - sp.tile0[s];
}

// stage rows r0 .. r0 + 63 of a sphere (`n` rows at `src`, `w` columns, w <= 64) into dst[64][AT_YP]; rows past the end and
// columns w .. 4 nst - 1 are zero
__device__ __forceinline__ void stage_rows(const float* __restrict__ src, int n, int r0, int w, int wpad, float (*dst)[AT_YP])
{
    for (int e = threadIdx.x; e < AT_TQ * wpad; e += 256) {
        const int r = e / wpad, c = e - r * wpad;
        dst[r][c] = (r0 + r < n && c < w) ? src[(int64_t)(r0 + r) * w + c] : 0.0f;
    }
}

// the 16 x 64 tile  own[16, 4 NST] . staged[64, 4 NST]^T  of one wave: s[t] holds rows 4 kk + r, column 16 t + i
template <int NST>
__device__ __forceinline__ void score_tile(const float (&xa)[NST], const float (*sy)[AT_YP], int i, int kk, f32x4v (&s)[4])
{
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        s[t] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int st = 0; st < NST; ++st) s[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[st], sy[16 * t + i][4 * st + kk], s[t], 0, 0, 0);
    }
}

// ---- forward (TR = 0) and dV (TR = 1) ----------------------------------------------------------------------------------
// TR = 0: own rows = queries (x = Q), streamed = keys (y = K, z = V), out = att (+ xn, lse)
// TR = 1: own rows = keys (x = K), streamed = queries (y = Q, z = dO), probabilities from the stored lse, out = dV
template <int TR, int NST, int CT>      // NST = MFMA steps over dq (dq <= 4 NST), CT = 16-column tiles of the dv slice
__global__ __launch_bounds__(256) void sphere_att_pv_kernel(AttSpheres sp, const float* __restrict__ x, const float* __restrict__ y,
                                                            const float* __restrict__ z, int dq, int dv, float* __restrict__ out,
                                                            float* __restrict__ xn, float* __restrict__ lse_out,
                                                            const float* __restrict__ lse_in)
{
    constexpr int SL = 16 * CT, ZP = SL + 16;        // 4 rows kk of a B read fall into 4 different groups of 16 banks
    __shared__ float sy[AT_TQ][AT_YP];
    __shared__ __attribute__((aligned(16))) float sz[AT_TQ][ZP];
    __shared__ float sp_[4][16][AT_YP];
    int base, n, tile;
    att_tile(sp, base, n, tile);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, kk = lane >> 4;
    const int r0 = tile * AT_TQ + wave * 16;         // first own row of the wave, inside the sphere
    const int c0 = blockIdx.y * SL;                  // first column of the slice
    const float* xs = x + (int64_t)base * dq;
    const float* ys = y + (int64_t)base * dq;
    const float* zs = z + (int64_t)base * dv;
    float xa[NST];
    {
        const int row = r0 + i < n ? r0 + i : n - 1;
#pragma unroll
        for (int st = 0; st < NST; ++st) xa[st] = (4 * st + kk) < dq ? xs[(int64_t)row * dq + 4 * st + kk] : 0.0f;
    }
    f32x4v acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct] = f32x4v{0.f, 0.f, 0.f, 0.f};
    float m[4], l[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; l[r] = 0.0f; }

    for (int k0 = 0; k0 < n; k0 += AT_TQ) {
        __syncthreads();
        stage_rows(ys, n, k0, dq, 4 * NST, sy);
        for (int e = threadIdx.x; e < AT_TQ * (SL / 4); e += 256) {
            const int r = e / (SL / 4), c4 = e - r * (SL / 4);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k0 + r < n) v = *reinterpret_cast<const float4*>(zs + (int64_t)(k0 + r) * dv + c0 + 4 * c4);
            *reinterpret_cast<float4*>(&sz[r][4 * c4]) = v;
        }
        __syncthreads();
        f32x4v s[4];
        score_tile<NST>(xa, sy, i, kk, s);
        if (TR == 0) {
            float mx[4], sc[4], rs[4];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (k0 + 16 * t + i >= n) s[t] = f32x4v{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                mx[r] = fmaxf(fmaxf(s[0][r], s[1][r]), fmaxf(s[2][r], s[3][r]));
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], o, 64));
                mx[r] = fmaxf(mx[r], m[r]);           // (finite: the first column of every key tile is inside the sphere)
                sc[r] = expf(m[r] - mx[r]);
                rs[r] = 0.0f;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = expf(s[t][r] - mx[r]);
                    rs[r] += p;
                    sp_[wave][4 * kk + r][16 * t + i] = p;
                }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) rs[r] += __shfl_xor(rs[r], o, 64);
                l[r] = l[r] * sc[r] + rs[r];
                m[r] = mx[r];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) acc[ct][r] *= sc[r];
            }
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int qrow = k0 + 16 * t + i;
                const float lq = qrow < n ? lse_in[base + qrow] : 0.0f;
#pragma unroll
                for (int r = 0; r < 4; ++r) sp_[wave][4 * kk + r][16 * t + i] = qrow < n ? expf(s[t][r] - lq) : 0.0f;
            }
        }
        lds_order();
        float pa[16];
#pragma unroll
        for (int st = 0; st < 16; ++st) pa[st] = sp_[wave][i][4 * st + kk];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int st = 0; st < 16; ++st)
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[st], sz[4 * st + kk][16 * ct + i], acc[ct], 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = r0 + 4 * kk + r;
        if (row >= n) continue;
        const int64_t o = (int64_t)(base + row) * dv + c0 + i;
        if (TR == 0) {
            const float inv = 1.0f / l[r];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const float a = acc[ct][r] * inv;
                out[o + 16 * ct] = a;
                xn[o + 16 * ct] = a / (float)n;
            }
            if (lse_out && blockIdx.y == 0 && i == 0) lse_out[base + row] = m[r] + logf(l[r]);
        } else {
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) out[o + 16 * ct] = acc[ct][r];
        }
    }
}

// ---- backward pre-pass: dO = d_att + d_xn / n, D = rowsum(dO o att); one wave per row -------------------------------------
__global__ __launch_bounds__(256) void sphere_att_pre_kernel(AttSpheres sp, int64_t nrows, int dv, const float* __restrict__ d_att,
                                                             const float* __restrict__ d_xn, const float* __restrict__ att,
                                                             float* __restrict__ d_o, float* __restrict__ dsum)
{
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows) return;
    int s = 0;
    while (s + 1 < sp.count && row >= sp.row0[s + 1]) ++s;
    const float nf = (float)(sp.row0[s + 1] - sp.row0[s]);
    float sum = 0.0f;
    for (int c = ws_lane(); c < dv; c += 64) {
        const int64_t o = row * dv + c;
        float g = d_att ? d_att[o] : 0.0f;
        if (d_xn) g += d_xn[o] / nf;
        d_o[o] = g;
        sum += g * att[o];
    }
    sum = ws_wave_sum(sum);
    if (ws_lane() == 0) dsum[row] = sum;
}

// ---- dQ (TR = 0) and dK (TR = 1) ---------------------------------------------------------------------------------------
// TR = 0: own rows = queries (x1 = Q, x2 = dO), streamed = keys (y1 = K, y2 = V):  dQ = (P o (dO V^T - D)) K, L / D by row
// TR = 1: own rows = keys (x1 = K, x2 = V), streamed = queries (y1 = Q, y2 = dO):  dK = dS^T Q, L / D by column
template <int TR, int NST>
__global__ __launch_bounds__(256) void sphere_att_dqk_kernel(AttSpheres sp, const float* __restrict__ x1, const float* __restrict__ y1,
                                                             const float* __restrict__ x2, const float* __restrict__ y2, int dq, int dv,
                                                             const float* __restrict__ lse, const float* __restrict__ dsum,
                                                             float* __restrict__ out)
{
    constexpr int OT = (4 * NST + 15) / 16;          // 16-column tiles of the [16, dq] output
    constexpr int VP = AT_DVC + 4;
    __shared__ float sy[AT_TQ][AT_YP];
    __shared__ __attribute__((aligned(16))) float sv[AT_TQ][VP];
    __shared__ float sp_[4][16][AT_YP];
    int base, n, tile;
    att_tile(sp, base, n, tile);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, kk = lane >> 4;
    const int r0 = tile * AT_TQ + wave * 16;
    const float* x1s = x1 + (int64_t)base * dq;
    const float* y1s = y1 + (int64_t)base * dq;
    const float* y2s = y2 + (int64_t)base * dv;
    const int arow = r0 + i < n ? r0 + i : n - 1;    // the row this lane feeds into A operands
    const float* x2r = x2 + (int64_t)(base + arow) * dv;
    float xa[NST];
#pragma unroll
    for (int st = 0; st < NST; ++st) xa[st] = (4 * st + kk) < dq ? x1s[(int64_t)arow * dq + 4 * st + kk] : 0.0f;
    float lrow[4], drow[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = r0 + 4 * kk + r < n ? r0 + 4 * kk + r : n - 1;
        lrow[r] = TR == 0 ? lse[base + row] : 0.0f;
        drow[r] = TR == 0 ? dsum[base + row] : 0.0f;
    }
    f32x4v acc[OT];
#pragma unroll
    for (int ot = 0; ot < OT; ++ot) acc[ot] = f32x4v{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < n; k0 += AT_TQ) {
        __syncthreads();
        stage_rows(y1s, n, k0, dq, 16 * OT, sy);
        f32x4v dp[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) dp[t] = f32x4v{0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < dv; c0 += AT_DVC) {
            const int cw = dv - c0 < AT_DVC ? dv - c0 : AT_DVC;     // 64 or 128 (dv % 64 == 0)
            if (c0 > 0) __syncthreads();
            for (int e = threadIdx.x; e < AT_TQ * (cw / 4); e += 256) {
                const int r = e / (cw / 4), c4 = e - r * (cw / 4);
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (k0 + r < n) v = *reinterpret_cast<const float4*>(y2s + (int64_t)(k0 + r) * dv + c0 + 4 * c4);
                *reinterpret_cast<float4*>(&sv[r][4 * c4]) = v;
            }
            __syncthreads();
            for (int st = 0; st < cw / 4; ++st) {
                const float a = x2r[c0 + 4 * st + kk];
#pragma unroll
                for (int t = 0; t < 4; ++t) dp[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, sv[16 * t + i][4 * st + kk], dp[t], 0, 0, 0);
            }
        }
        f32x4v s[4];
        score_tile<NST>(xa, sy, i, kk, s);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int col = k0 + 16 * t + i;
            const bool ok = col < n;
            const float lc = (TR == 1 && ok) ? lse[base + col] : 0.0f;
            const float dc = (TR == 1 && ok) ? dsum[base + col] : 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = expf(s[t][r] - (TR == 0 ? lrow[r] : lc));
                sp_[wave][4 * kk + r][16 * t + i] = ok ? p * (dp[t][r] - (TR == 0 ? drow[r] : dc)) : 0.0f;
            }
        }
        lds_order();
        float pa[16];
#pragma unroll
        for (int st = 0; st < 16; ++st) pa[st] = sp_[wave][i][4 * st + kk];
#pragma unroll
        for (int ot = 0; ot < OT; ++ot)
#pragma unroll
            for (int st = 0; st < 16; ++st)
                acc[ot] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[st], sy[4 * st + kk][16 * ot + i], acc[ot], 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = r0 + 4 * kk + r;
        if (row >= n) continue;
#pragma unroll
        for (int ot = 0; ot < OT; ++ot)
            if (16 * ot + i < dq) out[(int64_t)(base + row) * dq + 16 * ot + i] = acc[ot][r];
    }
}

// ---- channel form: row softmax of [rows, c] and its backward; one wave per row, c <= 512 ------------------------------------
constexpr int CH_PER = 8;              // elements per lane: c <= 512

__global__ __launch_bounds__(256) void channel_softmax_kernel(float* __restrict__ e, int64_t rows, int c, int max_minus)
{
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float* er = e + row * c;
    const int lane = ws_lane();
    float v[CH_PER];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < CH_PER; ++j) {
        const int col = lane + 64 * j;
        v[j] = col < c ? er[col] : -INFINITY;
        mx = fmaxf(mx, v[j]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (max_minus) {                   // t = rowmax(E) - E, then the softmax's own maximum (blocks.py:870-872)
        float tm = -INFINITY;
#pragma unroll
        for (int j = 0; j < CH_PER; ++j) {
            v[j] = (lane + 64 * j) < c ? mx - v[j] : -INFINITY;
            tm = fmaxf(tm, v[j]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tm = fmaxf(tm, __shfl_xor(tm, o, 64));
        mx = tm;
    }
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < CH_PER; ++j) {
        v[j] = (lane + 64 * j) < c ? expf(v[j] - mx) : 0.0f;
        sum += v[j];
    }
    sum = ws_wave_sum(sum);
#pragma unroll
    for (int j = 0; j < CH_PER; ++j)
        if (lane + 64 * j < c) er[lane + 64 * j] = v[j] / sum;
}

// dE = sign * A o (dA - rowsum(dA o A)), in place over dA; with at / det also A^T and dE^T of every [c, c] matrix
__global__ __launch_bounds__(256) void channel_softmax_bwd_kernel(const float* __restrict__ a, float* __restrict__ da, int64_t rows, int c,
                                                                  float sign, float* __restrict__ at, float* __restrict__ det)
{
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = ws_lane();
    const float* ar = a + row * c;
    float* dr = da + row * c;
    float av[CH_PER], dv[CH_PER];
    float dot = 0.0f;
#pragma unroll
    for (int j = 0; j < CH_PER; ++j) {
        const int col = lane + 64 * j;
        av[j] = col < c ? ar[col] : 0.0f;
        dv[j] = col < c ? dr[col] : 0.0f;
        dot += av[j] * dv[j];
    }
    dot = ws_wave_sum(dot);
    const int64_t mat = row / c;
    const int rin = (int)(row - mat * c);
#pragma unroll
    for (int j = 0; j < CH_PER; ++j) {
        const int col = lane + 64 * j;
        if (col >= c) continue;
        const float g = sign * (av[j] * (dv[j] - dot));
        dr[col] = g;
        if (at) {
            const int64_t o = mat * c * c + (int64_t)col * c + rin;
            at[o] = av[j];
            det[o] = g;
        }
    }
}

// host side ------------------------------------------------------------------------------------------------------------
int att_spheres(const int64_t* lengths, int32_t nspheres, int64_t n, AttSpheres& sp, int64_t& tiles)
{
    WS_REQUIRE(nspheres >= 0 && (lengths || nspheres == 0), "NULL lengths");
    int64_t sum = 0;
    for (int s = 0; s < nspheres; ++s) WS_REQUIRE(lengths[s] >= 0, "sphere %d: negative length %lld", s, (long long)lengths[s]);
    for (int s = 0; s < nspheres; ++s) {
        sum += lengths[s];
        WS_REQUIRE(sum <= n, "the sphere lengths sum to more than the %lld rows", (long long)n);
    }
    WS_REQUIRE(sum == n, "the sphere lengths sum to %lld, the operands hold %lld rows", (long long)sum, (long long)n);
    if (nspheres > AT_MAX_SPHERES)
        return ws_fail(WS_ERR_UNSUPPORTED, "%d spheres: the offsets travel in the kernel arguments, at most %d", nspheres, AT_MAX_SPHERES);
    if (n >= (1ll << 22))
        return ws_fail(WS_ERR_UNSUPPORTED, "%lld stacked rows: 32-bit element offsets need fewer than 2^22", (long long)n);
    sp = AttSpheres{};
    sp.count = nspheres;
    tiles = 0;
    int64_t row = 0;
    for (int s = 0; s < nspheres; ++s) {
        sp.row0[s] = (int32_t)row;
        sp.tile0[s] = (int32_t)tiles;
        row += lengths[s];
        tiles += ws_ceil_div(lengths[s], AT_TQ);
    }
    for (int s = nspheres; s <= AT_MAX_SPHERES; ++s) { sp.row0[s] = (int32_t)row; sp.tile0[s] = (int32_t)tiles; }
    return WS_OK;
}

int att_widths(int32_t dq, int32_t dv)
{
    WS_REQUIRE(dq >= 1 && dv >= 1, "bad widths dq=%d dv=%d", dq, dv);
    if (dq % 8 != 0 || dq > 64 || dv % 64 != 0 || dv > 512)
        return ws_fail(WS_ERR_UNSUPPORTED, "sphere attention takes dq %% 8 == 0, dq <= 64, dv %% 64 == 0, dv <= 512 (got dq=%d dv=%d)", dq, dv);
    return WS_OK;
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// both launchers: the launch and its check
template <int TR>
int launch_pv(const AttSpheres& sp, int64_t tiles, const float* x, const float* y, const float* z, int dq, int dv, float* out, float* xn,
              float* lse_out, const float* lse_in, hipStream_t st)
{
    const int nst = dq <= 8 ? 2 : dq <= 32 ? 8 : 16;
    const bool wide = dv % 128 == 0;
    const dim3 grid((unsigned)tiles, (unsigned)(dv / (wide ? 128 : 64)));
    const bool called = dispatch([&](auto ns, auto ct) {
        sphere_att_pv_kernel<TR, ns.value, ct.value><<<grid, 256, 0, st>>>(sp, x, y, z, dq, dv, out, xn, lse_out, lse_in);
    }, Pick<2, 8, 16>{nst}, Pick<4, 8>{wide ? 8 : 4});
    if (!called) return ws_no_instantiation("sphere_att_pv_kernel<TR=%d, NST=%d, CT=%d>", TR, nst, wide ? 8 : 4);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

template <int TR>
int launch_dqk(const AttSpheres& sp, int64_t tiles, const float* x1, const float* y1, const float* x2, const float* y2, int dq, int dv,
               const float* lse, const float* dsum, float* out, hipStream_t st)
{
    const int nst = dq <= 8 ? 2 : dq <= 32 ? 8 : 16;
    const bool called = dispatch([&](auto ns) {
        sphere_att_dqk_kernel<TR, ns.value><<<dim3((unsigned)tiles), 256, 0, st>>>(sp, x1, y1, x2, y2, dq, dv, lse, dsum, out);
    }, Pick<2, 8, 16>{nst});
    if (!called) return ws_no_instantiation("sphere_att_dqk_kernel<TR=%d, NST=%d>", TR, nst);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int channel_args(int64_t n, int32_t c, const int64_t* lengths, int32_t nspheres)
{
    WS_REQUIRE(n >= 0 && c >= 1, "bad sizes n=%lld c=%d", (long long)n, c);
    WS_REQUIRE(nspheres >= 0 && (lengths || nspheres == 0), "NULL lengths");
    int64_t sum = 0;
    for (int s = 0; s < nspheres; ++s) WS_REQUIRE(lengths[s] >= 0, "sphere %d: negative length %lld", s, (long long)lengths[s]);
    for (int s = 0; s < nspheres; ++s) {
        sum += lengths[s];
        WS_REQUIRE(sum <= n, "the sphere lengths sum to more than the %lld rows", (long long)n);
    }
    WS_REQUIRE(sum == n, "the sphere lengths sum to %lld, the operands hold %lld rows", (long long)sum, (long long)n);
    if (c % 4 != 0 || c > 64 * CH_PER)
        return ws_fail(WS_ERR_UNSUPPORTED, "channel attention takes c %% 4 == 0, c <= %d (got %d)", 64 * CH_PER, c);
    if (nspheres > AT_MAX_SPHERES)
        return ws_fail(WS_ERR_UNSUPPORTED, "%d spheres: at most %d per call", nspheres, AT_MAX_SPHERES);
    return WS_OK;
}

int64_t xty_bytes(int64_t m, int32_t c) { return (ws_gemm_xty_scratch_bytes(m, c, c) + 255) & ~255ll; }

}  // namespace

extern "C" {

int ws_sphere_attention_fwd(const float* q, const float* k, const float* v, int64_t n, int32_t dq, int32_t dv, const int64_t* lengths,
                            int32_t nspheres, float* att, float* xn, float* lse, void* stream)
{
    WS_REQUIRE(n >= 0, "bad row count %lld", (long long)n);
    int rc = att_widths(dq, dv);
    if (rc != WS_OK) return rc;
    AttSpheres sp;
    int64_t tiles;
    rc = att_spheres(lengths, nspheres, n, sp, tiles);
    if (rc != WS_OK) return rc;
    if (n == 0) return WS_OK;
    WS_REQUIRE(q && k && v && att && xn, "NULL argument");
    WS_REQUIRE(al16(v), "v must be 16-byte aligned");
    return launch_pv<0>(sp, tiles, q, k, v, dq, dv, att, xn, lse, nullptr, (hipStream_t)stream);
}

int64_t ws_sphere_attention_bwd_scratch_bytes(int64_t n, int32_t dv)
{
    if (n < 0 || dv < 1) return 0;
    return (n * (int64_t)dv + n) * (int64_t)sizeof(float) + 256;
}

int ws_sphere_attention_bwd(const float* q, const float* k, const float* v, const float* att, const float* lse, const float* d_att,
                            const float* d_xn, int64_t n, int32_t dq, int32_t dv, const int64_t* lengths, int32_t nspheres,
                            float* d_q, float* d_k, float* d_v, void* scratch, int64_t scratch_bytes, void* stream)
{
    WS_REQUIRE(n >= 0, "bad row count %lld", (long long)n);
    int rc = att_widths(dq, dv);
    if (rc != WS_OK) return rc;
    AttSpheres sp;
    int64_t tiles;
    rc = att_spheres(lengths, nspheres, n, sp, tiles);
    if (rc != WS_OK) return rc;
    if (n == 0) return WS_OK;
    WS_REQUIRE(q && k && v && att && lse && d_q && d_k && d_v && scratch, "NULL argument");
    WS_REQUIRE(d_att || d_xn, "NULL argument: no incoming gradient");
    if (scratch_bytes < ws_sphere_attention_bwd_scratch_bytes(n, dv))
        return ws_fail(WS_ERR_CAPACITY, "scratch too small: %lld < %lld bytes", (long long)scratch_bytes,
                       (long long)ws_sphere_attention_bwd_scratch_bytes(n, dv));
    float* d_o = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(scratch) + 255) & ~(uintptr_t)255);
    float* dsum = d_o + n * (int64_t)dv;
    WS_REQUIRE(al16(v), "v must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    sphere_att_pre_kernel<<<(unsigned)ws_ceil_div(n, 4), 256, 0, st>>>(sp, n, dv, d_att, d_xn, att, d_o, dsum);
    WS_LAUNCH_CHECK();
    rc = launch_dqk<0>(sp, tiles, q, k, d_o, v, dq, dv, lse, dsum, d_q, st);
    if (rc == WS_OK) rc = launch_pv<1>(sp, tiles, k, q, d_o, dq, dv, d_v, nullptr, nullptr, lse, st);
    if (rc == WS_OK) rc = launch_dqk<1>(sp, tiles, k, q, v, d_o, dq, dv, lse, dsum, d_k, st);
    return rc;
}

int64_t ws_channel_attention_scratch_bytes(const int64_t* lengths, int32_t nspheres, int32_t c, int32_t backward)
{
    if (!lengths || nspheres < 0 || c < 1) return 0;
    int64_t bytes = 256;
    for (int s = 0; s < nspheres; ++s) bytes += xty_bytes(lengths[s] > 0 ? lengths[s] : 0, c);
    if (backward) bytes += 3 * (((int64_t)nspheres * c * c * (int64_t)sizeof(float) + 255) & ~255ll);   // dA / dE, A^T, dE^T
    return bytes;
}

int ws_channel_attention_fwd(const float* x1, const float* x2, const float* value, int64_t n, int32_t c, const int64_t* lengths,
                             int32_t nspheres, int32_t max_minus, float* a, float* out, void* scratch, int64_t scratch_bytes,
                             void* stream)
{
    const int rc = channel_args(n, c, lengths, nspheres);
    if (rc != WS_OK) return rc;
    if (nspheres == 0) return WS_OK;
    WS_REQUIRE(a && scratch && (n == 0 || (x1 && x2 && value && out)), "NULL argument");
    if (scratch_bytes < ws_channel_attention_scratch_bytes(lengths, nspheres, c, 0))
        return ws_fail(WS_ERR_CAPACITY, "scratch too small: %lld < %lld bytes", (long long)scratch_bytes,
                       (long long)ws_channel_attention_scratch_bytes(lengths, nspheres, c, 0));
    char* sc = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(scratch) + 255) & ~(uintptr_t)255);
    ws_xty_problem ep[AT_MAX_SPHERES];
    ws_xb_problem op[AT_MAX_SPHERES];
    int64_t row = 0;
    for (int s = 0; s < nspheres; ++s) {
        const int64_t m = lengths[s];
        ep[s] = ws_xty_problem{x1 + row * c, m, c, c, x2 + row * c, c, c, a + (int64_t)s * c * c, 0, sc, xty_bytes(m, c)};
        sc += xty_bytes(m, c);
        op[s] = ws_xb_problem{};
        op[s].x = value + row * c; op[s].m = m; op[s].k = c; op[s].ldx = c;
        op[s].b = a + (int64_t)s * c * c; op[s].b_row_stride = -1; op[s].b_col_stride = 1; op[s].n = c;
        op[s].y = out + row * c; op[s].ldy = c;
        row += m;
    }
    int r = ws_priv_gemm_xty_group(ep, nspheres, stream);
    if (r != WS_OK) return r;
    const int64_t rows = (int64_t)nspheres * c;
    channel_softmax_kernel<<<(unsigned)ws_ceil_div(rows, 4), 256, 0, (hipStream_t)stream>>>(a, rows, c, max_minus ? 1 : 0);
    WS_LAUNCH_CHECK();
    return ws_priv_gemm_xb_group(op, nspheres, stream);
}

int ws_channel_attention_bwd(const float* x1, const float* x2, const float* value, const float* a, const float* d_out, int64_t n,
                             int32_t c, const int64_t* lengths, int32_t nspheres, int32_t max_minus, float* d_x1, float* d_x2,
                             float* d_value, void* scratch, int64_t scratch_bytes, void* stream)
{
    const int rc = channel_args(n, c, lengths, nspheres);
    if (rc != WS_OK) return rc;
    if (nspheres == 0) return WS_OK;
    WS_REQUIRE(a && scratch && (n == 0 || (x1 && x2 && value && d_out && d_x1 && d_x2 && d_value)), "NULL argument");
    if (scratch_bytes < ws_channel_attention_scratch_bytes(lengths, nspheres, c, 1))
        return ws_fail(WS_ERR_CAPACITY, "scratch too small: %lld < %lld bytes", (long long)scratch_bytes,
                       (long long)ws_channel_attention_scratch_bytes(lengths, nspheres, c, 1));
    char* sc = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(scratch) + 255) & ~(uintptr_t)255);
    const int64_t mat_bytes = ((int64_t)nspheres * c * c * (int64_t)sizeof(float) + 255) & ~255ll;
    float* d_e = reinterpret_cast<float*>(sc);
    float* a_t = reinterpret_cast<float*>(sc + mat_bytes);
    float* d_et = reinterpret_cast<float*>(sc + 2 * mat_bytes);
    sc += 3 * mat_bytes;
    const bool strided = c % 32 == 0;                // the MFMA product reads a transposed B through its strides
    ws_xty_problem ep[AT_MAX_SPHERES];
    int64_t row = 0;
    for (int s = 0; s < nspheres; ++s) {
        const int64_t m = lengths[s];
        ep[s] = ws_xty_problem{value + row * c, m, c, c, d_out + row * c, c, c, d_e + (int64_t)s * c * c, 0, sc, xty_bytes(m, c)};
        sc += xty_bytes(m, c);
        row += m;
    }
    int r = ws_priv_gemm_xty_group(ep, nspheres, stream);
    if (r != WS_OK) return r;
    const int64_t rows = (int64_t)nspheres * c;
    channel_softmax_bwd_kernel<<<(unsigned)ws_ceil_div(rows, 4), 256, 0, (hipStream_t)stream>>>(a, d_e, rows, c, max_minus ? -1.0f : 1.0f,
                                                                                              strided ? nullptr : a_t,
                                                                                              strided ? nullptr : d_et);
    WS_LAUNCH_CHECK();
    // dVal = dOut A^T, dX1 = X2 dE^T, dX2 = X1 dE: one list, grouped by the product's own rules
    ws_xb_problem op[3 * AT_MAX_SPHERES];
    for (int part = 0; part < 3; ++part) {
        row = 0;
        for (int s = 0; s < nspheres; ++s) {
            const int64_t m = lengths[s], mo = (int64_t)s * c * c;
            ws_xb_problem& p = op[part * nspheres + s];
            p = ws_xb_problem{};
            p.m = m; p.k = c; p.ldx = c; p.n = c; p.ldy = c;
            p.b_row_stride = -1; p.b_col_stride = 1;
            if (part == 0) { p.x = d_out + row * c; p.b = strided ? a + mo : a_t + mo; p.y = d_value + row * c; }
            else if (part == 1) { p.x = x2 + row * c; p.b = strided ? d_e + mo : d_et + mo; p.y = d_x1 + row * c; }
            else { p.x = x1 + row * c; p.b = d_e + mo; p.y = d_x2 + row * c; }
            if (part < 2 && strided) { p.b_row_stride = 1; p.b_col_stride = c; }
            row += m;
        }
    }
    return ws_priv_gemm_xb_group(op, 3 * nspheres, stream);
}

}  // extern "C"
