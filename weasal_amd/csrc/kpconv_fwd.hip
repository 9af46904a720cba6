// weasal_amd/csrc/kpconv_fwd.hip -- the forward KPConv gather kernels for gfx950 (wave64) and their launches.
//
// K3  kpconv_gather_fwd :  wf[q,k,c] = sum_h w(q,h,k) * x[inds[q,h], c]
//     neighbour gather -> kernel-point influence -> feature aggregate in ONE kernel; the
//     [N,H,3] / [N,H,K,3] / [N,H,K] / [N,H,Ci] intermediates of the reference never exist.
// Two forms: the entry pool in LDS with a branch-free VALU flush (kpconv_gather_fwd_kernel; the pool and its list phase are
// in kpconv_device.h) and the matrix-core form (kpconv_gather_fwd_mfma_kernel), which also carries the fused forward layer.
#include "kpconv_launch.h"
#include "ws_dispatch.h"

namespace {

// ---------------------------------------------------------------------------------------------
// K3 forward.  In the flush phase entry slot s owns the kernel points s, s+S, s+2S, ...: it walks
// their segments with a float4 register accumulator and stores the finished 16-byte piece of
// wf[q,k,:] straight to HBM (fixed summation order).  The pool is built once per 64-column chunk
// and flushed for every 4*G-channel chunk; further column chunks (H > 64) and overflow sub-chunks
// accumulate onto the rows already written.  The index and xyz loads of the next two items are
// software-prefetched under the current item.
// ---------------------------------------------------------------------------------------------
template <int K, int G, int MODE, bool DEF, bool VEC, int PW = 4, typename T = float>
__global__ __launch_bounds__(256) void kpconv_gather_fwd_kernel(
    const float* __restrict__ q_pts, int64_t nq, const float* __restrict__ s_pts, int64_t ns,
    const int64_t* __restrict__ inds, int h, const T* __restrict__ x, int ci,
    const float* __restrict__ kernel_points, const float* __restrict__ deformed_kp,
    const float* __restrict__ modulations, GeomParams g, T* __restrict__ wf,
    float* __restrict__ min_d2, const int32_t* __restrict__ order)
{
    static_assert(!(DEF && MODE == 0), "deformable layers use MODE 1");
    static_assert(PW == 4 || (PW == 1 && !VEC), "piece width: 16 bytes, or one float for the 3-channel input layer");
    constexpr int CC = PW * G;     // channels per chunk (PW = 1: lane = (kernel point, channel), 4-byte pieces)
    constexpr int S = 64 / G;      // entry slots
    constexpr int KPS = (K + S - 1) / S;   // kernel points per slot
    static_assert(K <= 16 && POOL >= 16 * K, "pool sizing");
    __shared__ uint2 pool_all[4][POOL_ALLOC];
    __shared__ int segs_all[4][K + 1];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    uint2* pool = pool_all[wave];
    int* segs = segs_all[wave];
    const int j = lane % G;        // 16-byte piece of the row chunk
    const int slot = lane / G;
    const float inv_extent = 1.0f / g.extent;

    int64_t ibeg, iend;
    ws_block_range(nq, ibeg, iend);

    // MODE 0: the rigid kernel points are wave-uniform for the whole launch -> registers (SGPRs)
    float kpr[MODE == 0 ? 3 * K : 1];
    float cut2_pool = 3.4e38f;
    if (MODE == 0) {
#pragma unroll
        for (int t = 0; t < 3 * K; ++t) kpr[t] = kernel_points[t];
        if (g.cut) {
            float rr = 0.0f;
#pragma unroll
            for (int k = 0; k < K; ++k) rr = fmaxf(rr, (kpr[3 * k] * kpr[3 * k] + kpr[3 * k + 1] * kpr[3 * k + 1]) + kpr[3 * k + 2] * kpr[3 * k + 2]);
            const float R = (__builtin_sqrtf(rr) + g.extent) * 1.0001f;
            cut2_pool = R * R;
        }
    }

    // bf16 rows: the running sum of a row that takes several flushes (H > 64, pool overflow) stays in f32 registers and is
    // rounded once per store -- read back from wf it would be rounded to bf16 at every flush.  One channel chunk per lane
    // (the launcher sends ci <= 4 = CC here), so one float4 per kernel point of the slot.
    constexpr bool CARRY = sizeof(T) == 2;
    float4 carry[CARRY ? KPS : 1];
#pragma unroll
    for (int t = 0; t < (CARRY ? KPS : 1); ++t) carry[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    // flush the pool: every slot walks the segments of its kernel points for all channel chunks.
    // maxlen = longest segment (wave-uniform): every round runs that many steps.
    auto flush = [&](int64_t q, bool accumulate, int maxlen) {
        wave_lds_sync();
        if (PW == 1) {
            // narrow rows (the 3-channel input layer): one float per lane, a slot of G lanes per kernel point --
            // 45 of 64 lanes busy with one 4-byte load per entry instead of 15 lanes with four clamped loads
            for (int cc0 = 0; cc0 < ci; cc0 += CC) {
                const int ch = cc0 + j;
                const bool chok = ch < ci;
                const int chl = chok ? ch : 0;
#pragma unroll
                for (int kk = 0; kk < KPS; ++kk) {
                    const int k = slot + kk * S;
                    const bool kok = k < K && chok;
                    const int beg = kok ? segs[k] : 0;
                    const int end = kok ? min(segs[k + 1], POOL) : 0;
                    float a = 0.0f;
                    for (int it = 0; it < maxlen; it += 4) {
                        uint2 e[4];
                        float v[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            e[u] = pool[min(beg + it + u, POOL + 7)];
                            keep_unconditional(e[u]);
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const bool ok = beg + it + u < end;
                            e[u].x = ok ? e[u].x : 0u;
                            e[u].y = ok ? e[u].y : 0u;
                            v[u] = ld1(x + (size_t)(e[u].x * (unsigned)ci) + chl);
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u) a = fmaf(__uint_as_float(e[u].y), v[u], a);
                    }
                    if (kok) {
                        if (modulations) a *= modulations[q * K + k];
                        T* dst = wf + (q * K + k) * ci + ch;
                        st1(dst, (accumulate ? ld1(dst) : 0.f) + a);
                    }
                }
            }
            wave_lds_sync();
            return;
        }
        for (int cc0 = 0; cc0 < ci; cc0 += CC) {
            const int ch = cc0 + 4 * j;
            const bool chok = VEC ? (ch + 3 < ci) : (ch < ci);
            const int chl = chok ? ch : 0;
#pragma unroll
            for (int kk = 0; kk < KPS; ++kk) {
                const int k = slot + kk * S;
                const bool kok = k < K && chok;
                const int beg = kok ? segs[k] : 0;
                const int end = kok ? min(segs[k + 1], POOL) : 0;
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
                for (int it = 0; it < maxlen; it += 4) {
                    uint2 e[4];
                    float4 v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        e[u] = pool[min(beg + it + u, POOL + 7)];
                        keep_unconditional(e[u]);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const bool ok = beg + it + u < end;
                        e[u].x = ok ? e[u].x : 0u;
                        e[u].y = ok ? e[u].y : 0u;                    // weight 0.0f
                        v[u] = load_row_piece<VEC>(x, e[u].x, ci, chl);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float w = __uint_as_float(e[u].y);
                        a.x = fmaf(w, v[u].x, a.x); a.y = fmaf(w, v[u].y, a.y);
                        a.z = fmaf(w, v[u].z, a.z); a.w = fmaf(w, v[u].w, a.w);
                    }
                }
                if (kok) {
                    if (modulations) { const float md = modulations[q * K + k]; a.x *= md; a.y *= md; a.z *= md; a.w *= md; }
                    T* dst = wf + (q * K + k) * ci + ch;
                    if (VEC) {
                        if (accumulate) {
                            const float4 o = CARRY ? carry[CARRY ? kk : 0] : ld4(dst);
                            a.x += o.x; a.y += o.y; a.z += o.z; a.w += o.w;
                        }
                        if (CARRY) carry[CARRY ? kk : 0] = a;
                        st4(dst, a);
                    } else {
                        if (ch + 0 < ci) st1(dst + 0, (accumulate ? ld1(dst + 0) : 0.f) + a.x);
                        if (ch + 1 < ci) st1(dst + 1, (accumulate ? ld1(dst + 1) : 0.f) + a.y);
                        if (ch + 2 < ci) st1(dst + 2, (accumulate ? ld1(dst + 2) : 0.f) + a.z);
                        if (ch + 3 < ci) st1(dst + 3, (accumulate ? ld1(dst + 3) : 0.f) + a.w);
                    }
                }
            }
        }
        wave_lds_sync();
    };

    // ---- software pipeline over the items of this wave: idx two items ahead, xyz one item ahead
    auto item_q = [&](int64_t it) -> int64_t { return it < iend ? (order ? (int64_t)order[it] : it) : -1; };
    auto load_idx = [&](int64_t q) -> int {
        if (q < 0 || lane >= h) return -1;
        const int64_t v = inds[q * h + lane];
        return (v >= 0 && v < ns) ? (int)v : -1;
    };
    auto load_pt = [&](int idx, float& px, float& py, float& pz) {
        px = py = pz = WS_SHADOW;
        if (idx >= 0) { px = s_pts[3 * (int64_t)idx]; py = s_pts[3 * (int64_t)idx + 1]; pz = s_pts[3 * (int64_t)idx + 2]; }
    };
    int64_t q0 = item_q(ibeg + wave), q1 = item_q(ibeg + wave + 4);
    int idx0 = load_idx(q0), idx1 = load_idx(q1);
    float p0x, p0y, p0z;
    load_pt(idx0, p0x, p0y, p0z);

    for (int64_t item = ibeg + wave; item < iend; item += 4) {
        const int64_t q = q0;
        const int64_t q2 = item_q(item + 8);
        const int idx2 = load_idx(q2);
        float p1x, p1y, p1z;
        load_pt(idx1, p1x, p1y, p1z);

        const float qx = q_pts[3 * q + 0], qy = q_pts[3 * q + 1], qz = q_pts[3 * q + 2];
        const float* kpp = DEF ? deformed_kp + q * (3 * K) : kernel_points;      // wave-uniform
        auto kp = [&](int k, int c) { return MODE == 0 ? kpr[MODE == 0 ? 3 * k + c : 0] : kpp[3 * k + c]; };
        bool accumulate = false;
        for (int h0 = 0; h0 < h; h0 += 64) {
            const int col = h0 + lane;
            const bool incol = col < h;
            int idx = idx0;
            float px = p0x, py = p0y, pz = p0z;
            if (h0 > 0) {      // further column chunks are loaded on demand
                idx = -1;
                if (incol) { const int64_t v = inds[q * h + col]; idx = (v >= 0 && v < ns) ? (int)v : -1; }
                load_pt(idx, px, py, pz);
            }
            const bool real = incol && idx >= 0;
            const float nx = px - qx, ny = py - qy, nz = pz - qz;
            if (MODE == 0 && g.cut && h0 > 0) {
                // sorted rows: once a chunk holds no neighbour inside the influence reach, neither does any later one
                if (__ballot(real && (nx * nx + ny * ny) + nz * nz <= cut2_pool) == 0ull) break;
            }
            const unsigned row = (unsigned)(real ? idx : 0);
            int total = 0, maxlen = 0;
            if (MODE == 0 && h - h0 > 64) {
                // 65..128 columns left: both chunks into one pool, one flush
                const int colb = col + 64;
                int idxb = -1;
                if (colb < h) { const int64_t v = inds[q * h + colb]; idxb = (v >= 0 && v < ns) ? (int)v : -1; }
                float bx, by, bz;
                load_pt(idxb, bx, by, bz);
                const bool realb = idxb >= 0;
                kp_list2<K>(nx, ny, nz, real, row, bx - qx, by - qy, bz - qz, realb, (unsigned)(realb ? idxb : 0), kp, inv_extent,
                            pool, segs, lane, total, maxlen);
                if (total <= POOL) {
                    flush(q, accumulate, maxlen);
                    accumulate = true;
                    h0 += 64;
                    continue;
                }
                total = 0; maxlen = 0;      // does not fit: fall through, one chunk at a time
            }
            auto minf = [&](int k, float d) {
                if (DEF && min_d2) {
                    float m = incol ? d : 3.4e38f;
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o, 64));
                    if (lane == 0) min_d2[q * K + k] = h0 == 0 ? m : fminf(min_d2[q * K + k], m);
                }
            };
            kp_list<K, MODE>(nx, ny, nz, real, kp, g, inv_extent, row, 0u, nullptr, pool, segs, lane, total, maxlen, minf);
            if (total <= POOL) {
                flush(q, accumulate, maxlen);
                accumulate = true;
            } else {
                // the chunk does not fit the pool: redo it in four 16-lane sub-chunks (16 * K <= POOL)
                auto nomin = [&](int, float) {};
                for (int sub = 0; sub < 4; ++sub) {
                    total = 0; maxlen = 0;
                    kp_list<K, MODE>(nx, ny, nz, real && (lane >> 4) == sub, kp, g, inv_extent, row, 0u, nullptr, pool, segs,
                                     lane, total, maxlen, nomin);
                    flush(q, accumulate, maxlen);
                    accumulate = true;
                }
            }
        }
        // rotate the pipeline
        q0 = q1; q1 = q2;
        idx0 = idx1; idx1 = idx2;
        p0x = p1x; p0y = p1y; p0z = p1z;
    }
}

// ---------------------------------------------------------------------------------------------
// K3 forward on the matrix core.  The weighted-feature product of the reference,
//     weighted_features = torch.matmul(all_weights [N,K,H], neighb_x [N,H,Ci])       (models/blocks.py:363)
// is a small dense matrix product per query: wf[q] (15 x Ci) = W_q^T (15 x H) . X_q (H x Ci).  Here it runs as such on
// v_mfma_f32_16x16x4_f32 (exact f32: a k-ordered fmaf chain, so the sum over the neighbour columns has the same bits as
// the per-kernel-point VALU chains of kpconv_gather_fwd_kernel -- zero weights add exactly nothing):
//   A operand  A[i][k]   lane (i = lane&15, kk = lane>>4) holds the influence of kernel point i on neighbour column
//              4 s + kk of step s: ONE weight, computed by that lane from the neighbour's offset (an LDS broadcast of
//              the staged float4) and its own kernel point (rigid: a register for the whole launch; deformed: 3 loads
//              per query).  No ballot, no compaction, no entry pool: 16 steps x ~10 VALU per 64 columns.
//   B operand  B[k][j]   lane (j = lane&15, kk) loads NT consecutive channels of row inds[q, 4 s + kk] (one 4..64-byte
//              load; the 16 lanes of a row cover 16 NT channels = the whole row for Ci <= 256), tile t = channel
//              NT j + t; loads of a whole group of steps are in flight before the first MFMA needs them.
//   C / D      lane (j, g = lane>>4) ends with kernel points 4 g .. 4 g + 3 of channels NT j .. NT j + NT - 1: rows of wf
//              are written as contiguous 16 NT-channel runs.
// Wider rows (H > 64) simply keep accumulating over further 64-column chunks: no read-modify-write of wf.  Only ~1.3 of
// the 15 influences per neighbour are non-zero, so the matrix core does ~12 x the useful flops -- on a pipe that is
// otherwise idle here, at 32 cycles per 16x16x4 step: 30 MFMAs per query at Ci = 32 against the ~750 VALU/SALU/LDS
// instructions of the pool form.  MODE / DEF as above (MODE 0 = rigid, linear, sum).
// ---------------------------------------------------------------------------------------------
#ifndef WS_K3_GS
#define WS_K3_GS 4
#endif
#ifndef WS_FUSE_GS
#define WS_FUSE_GS 2      // steps in flight of the fused-contraction variant: its 60 registers of W leave room for fewer
#endif

// VECROW: ci is a multiple of NT and rows are aligned for NT-element accesses (else NT == 1 with per-lane masking)
// CUT (MODE 0 / 2 only): the caller vouches that every index row is sorted by distance from its query (what the radius search
// delivers, neighbors.cpp:293).  A neighbour farther from the query than  max_k |kp_k| + extent  has 15 zero influences, and
// one farther than  max_k (sqrt(min_d2[k] so far) + |kp_k|)  cannot lower any minimum (triangle inequality): the walk over
// the row stops there.  Exact -- the skipped terms are zeros -- and decisive where the rows come from the DEFORMABLE radius
// (datasets/common.py:500-502: 2 r, while the kernel points reach 0.69 r + extent = 1.09 r: 84 % of a rigid offset
// convolution's neighbours, ~60 % of a deformed one's, are outside every influence).
// FUSE (forward only; MODE 0, NT = 2, f32, Ci = Co = 32: the level-0 layers, where the time is): the kernel contraction
//   out[q, :] = act(wf[q] (1 x 15 Ci) . W (15 Ci x Co) + bias)                         (models/blocks.py:370-374, 556-563)
// runs inside this kernel and `wf` never reaches memory (N x 15 x Ci x 4 B = 768 MB at enc1, written and read back by the
// two-launch form -- which training keeps, dW needs wf).  The four waves of a workgroup gather one query each per
// iteration into an LDS tile of 16 queries (four iterations); then every wave multiplies its QUARTER of the 480-deep
// contraction -- that quarter of W lives in its registers for the whole launch (60 VGPRs: lane (j, kk) holds
// W[120 w + 4 s + kk][16 n + j]) -- on v_mfma_f32_16x16x4_f32, the four partial [16 x 32] tiles are added through LDS
// with the bias / LeakyReLU epilogue and stored as 16 output rows.  Tile rows are 484 floats apart: the A-operand reads
// (lane (query, kk)) fall on 64 different banks.
template <int NT, int MODE, bool DEF, bool VECROW, typename T, int GSV = 0, bool CUT = false, bool FUSE = false, int K = 15>
__global__ __launch_bounds__(256) void kpconv_gather_fwd_mfma_kernel(
    const float* __restrict__ q_pts, int64_t nq, const float* __restrict__ s_pts, int64_t ns,
    const int64_t* __restrict__ inds, int h, const T* __restrict__ x, int ci,
    const float* __restrict__ kernel_points, const float* __restrict__ deformed_kp,
    const float* __restrict__ modulations, GeomParams g, T* __restrict__ wf,
    float* __restrict__ min_d2, const int32_t* __restrict__ order, FuseArgs fz = FuseArgs{})
{
    static_assert(!FUSE || (MODE == 0 && NT == 2 && sizeof(T) == 4 && VECROW && K == 15), "the fused contraction covers rigid 32 -> 32 f32 layers of 15 kernel points");
    static_assert(K >= 1 && K <= 16, "the kernel points are the rows of ONE 16-row A tile; rows >= K are masked");
    constexpr int TILE_LD = 484;
    constexpr int CB = 16 * NT;                                   // channels per block
    // steps whose loads are in flight together (per buffer; two buffers): more = deeper memory pipelining per wave,
    // fewer = fewer registers = more waves per SIMD.  The kernel is bound by instruction latency x occupancy (with every
    // memory access ablated it still takes 0.53 of its 0.68 ms on the 400k x 59 x 32 layer), so registers win
    constexpr int GS = GSV > 0 ? GSV : (NT <= 2 ? WS_K3_GS : (NT == 4 ? 2 : 1));
    static_assert(!(DEF && MODE == 0), "deformable layers use MODE 1 or 2");
    static_assert(MODE != 2 || DEF, "MODE 2 is the deformable fast path");
    static_assert(!CUT || MODE == 0 || MODE == 2, "the distance cutoff belongs to the linear-influence fast paths");
    static_assert(VECROW || NT == 1, "masked rows use one channel per lane");
    __shared__ float4 nb_all[4][64];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int i = lane & 15, kk = lane >> 4;                      // A: kernel point i; B / D: channel lane j = i; row group kk
    float4* nb = nb_all[wave];
    const float inv_extent = 1.0f / g.extent;
    const float e2 = g.extent * g.extent;
    const bool haskp = i < K;

    const int csplit = (FUSE || MODE != 0 || g.csplit < 1) ? 1 : g.csplit;      // items per query (see GeomParams::csplit)
    int64_t ibeg, iend;
    ws_block_range(nq * csplit, ibeg, iend);

    float kx = 0.f, ky = 0.f, kz = 0.f;
    if (!DEF && haskp) { kx = kernel_points[3 * i]; ky = kernel_points[3 * i + 1]; kz = kernel_points[3 * i + 2]; }
    if ((MODE == 0 || MODE == 2) && !haskp) kx = ky = kz = 1.0e9f;   // the 16th "kernel point": far from everything, weight 0
    float kmod = 0.0f;                                            // MODE 2: modulation of this lane's kernel point
    // squared cutoff on the neighbour's distance from the query (CUT); rigid: a constant of the launch
    auto group_max = [&](float v) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
        return v;
    };
    float cut2_rigid = 3.4e38f;
    if constexpr (CUT && MODE == 0) {
        const float rr = group_max(haskp ? __builtin_sqrtf((kx * kx + ky * ky) + kz * kz) : 0.0f);
        const float R = (rr + g.extent) * 1.0001f;
        cut2_rigid = R * R;
    }

    // ---- software pipeline over the items of this wave.  Everything an item needs before its row loads -- its query index
    // (order[]), its index row, the neighbours' coordinates, its own coordinates -- is a chain of dependent memory
    // accesses of ~1 us each; executed at the item they would leave the wave idle for several microseconds per query (the
    // first forms of this kernel spent 0.47 of 0.68 ms with EVERY memory access and all arithmetic ablated).  So the chain
    // is spread over three items: at the top of item t the wave issues  order[t+3],  inds / q_pts of item t+2,  the
    // neighbour coordinates of item t+1,  and looks at none of the results before the next iteration.  All of them are
    // VECTOR loads, also the lane-uniform ones (order, q_pts: the address carries an opaque zero VGPR): scalar loads share
    // the lgkm counter with LDS and return out of order, so the LDS ordering below would wait for them on the spot.
    int vz;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vz));
    const int64_t it0 = ibeg + wave;
    if (FUSE ? (ibeg >= iend) : (it0 >= iend)) return;            // (FUSE: workgroup-uniform -- every wave meets the barriers)
    // FUSE: every wave runs the same number of iterations (dummy ones redo the workgroup's last query and store nothing)
    const int64_t iend_u = FUSE ? ibeg + ((iend - ibeg + 3) / 4) * 4 : iend;
    float wq[FUSE ? 30 : 1][2];
    if constexpr (FUSE) {
#pragma unroll
        for (int s_ = 0; s_ < 30; ++s_) {
            wq[s_][0] = fz.w[(120 * wave + 4 * s_ + kk) * 32 + i];
            wq[s_][1] = fz.w[(120 * wave + 4 * s_ + kk) * 32 + 16 + i];
        }
    }
    int iter = 0;
    auto item_v = [&](int64_t it) -> int {                        // query of item `it`, in a VGPR (clamped past the end)
        const int64_t itc = it < iend ? it : iend - 1;
        const int64_t qi = csplit > 1 ? itc / csplit : itc;
        return order ? order[qi + vz] : (int)qi + vz;
    };
    const int col0 = lane < h ? lane : 0;
    auto raw_idx = [&](int qv) -> int64_t { return inds[(int64_t)qv * h + col0]; };
    auto chk = [&](int64_t raw) -> int { return (lane < h && raw >= 0 && raw < ns) ? (int)raw : -1; };
    auto pt_raw = [&](int idx, float& px, float& py, float& pz) {
        const int ii = idx >= 0 ? idx : 0;
        px = s_pts[3 * (int64_t)ii]; py = s_pts[3 * (int64_t)ii + 1]; pz = s_pts[3 * (int64_t)ii + 2];
    };
    auto q_xyz = [&](int qv, float& x_, float& y_, float& z_) {
        x_ = q_pts[3 * (int64_t)qv + 0]; y_ = q_pts[3 * (int64_t)qv + 1]; z_ = q_pts[3 * (int64_t)qv + 2];
    };
    auto load_idx = [&](int qv, int col) -> int {                  // (further 64-column chunks of wide rows: at use)
        if (col >= h) return -1;
        const int64_t v = inds[(int64_t)qv * h + col];
        return (v >= 0 && v < ns) ? (int)v : -1;
    };
    auto load_pt = [&](int idx, float& px, float& py, float& pz) {
        px = py = pz = WS_SHADOW;
        if (idx >= 0) { px = s_pts[3 * (int64_t)idx]; py = s_pts[3 * (int64_t)idx + 1]; pz = s_pts[3 * (int64_t)idx + 2]; }
    };
    int qv0 = item_v(it0), qv1 = item_v(it0 + 4), qv2 = item_v(it0 + 8);
    int64_t raw1 = raw_idx(qv1);
    int idx0 = chk(raw_idx(qv0));
    float p0x, p0y, p0z, qx, qy, qz, q1x, q1y, q1z;
    pt_raw(idx0, p0x, p0y, p0z);
    p0x = idx0 >= 0 ? p0x : WS_SHADOW; p0y = idx0 >= 0 ? p0y : WS_SHADOW; p0z = idx0 >= 0 ? p0z : WS_SHADOW;
    q_xyz(qv0, qx, qy, qz);
    q_xyz(qv1, q1x, q1y, q1z);
    int idx1 = chk(raw1);

    for (int64_t item = it0; item < iend_u; item += 4) {
        const int64_t q = qv0;                                    // (a VGPR value, the same in every lane)
        const int qv3 = item_v(item + 12);
        const int64_t raw2 = raw_idx(qv2);
        float q2x, q2y, q2z, p1x, p1y, p1z;
        q_xyz(qv2, q2x, q2y, q2z);
        pt_raw(idx1, p1x, p1y, p1z);
        if constexpr (MODE == 2) {
            if (haskp) {
                const float4 kq = g.kp4[q * K + i];
                kx = kq.x; ky = kq.y; kz = kq.z; kmod = kq.w;
            }
        } else if (DEF && haskp) {
            const float* kp = deformed_kp + q * (3 * K) + 3 * i;
            kx = kp[0]; ky = kp[1]; kz = kp[2];
        }
        // channel blocks of this item: all of them, or the item's run of whole blocks
        int cb_lo = 0, cb_hi = ci;
        if (csplit > 1) {
            const int run = ((ci + CB * csplit - 1) / (CB * csplit)) * CB;
            cb_lo = (int)(item % csplit) * run;
            cb_hi = min(ci, cb_lo + run);
        }
        float mind = 3.4e38f;
        float cut2 = cut2_rigid, rk = 0.0f, rq = 0.0f;
        if constexpr (CUT && MODE == 2) {
            rk = haskp ? __builtin_sqrtf((kx * kx + ky * ky) + kz * kz) : 0.0f;
            rq = group_max(rk) + g.extent;                            // beyond it: no influence
            cut2 = 3.4e38f;                                           // the first chunk is walked in full (min_d2 needs a start)
        }
        for (int cb = cb_lo; cb < cb_hi; cb += CB) {
            f32x4v acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = f32x4v{0.f, 0.f, 0.f, 0.f};
            const int ch = cb + NT * i;                           // first channel of this lane
            const bool chok = VECROW ? (ch < ci) : (ch < ci);
            for (int h0 = 0; h0 < h; h0 += 64) {
                int idx = idx0;
                float px = p0x, py = p0y, pz = p0z;
                if (h0 > 0) {
                    idx = load_idx(qv0, h0 + lane);
                    load_pt(idx, px, py, pz);
                }
                wave_lds_order();                                 // the previous chunk's readers are done
                if constexpr (MODE == 0 || MODE == 2) {
                    // ---- MODE 2 (deformable + modulated, linear, sum; BASELINE config 5) shares this form: the lane's kernel
                    // point is re-loaded per query (one float4 with its modulation), the modulation multiplies the influence
                    // (A operand) instead of the finished row, min_d2 is tracked per lane.  The in-range filter of
                    // blocks.py:301-325 needs no code here: with the linear influence a neighbour without a kernel point
                    // inside the extent has all 15 influences equal to zero already.  Columns past the row are staged
                    // far beyond the shadow point so that they never win the minimum; shadow columns take part in it with
                    // the reference's coordinates (1e6 - q, blocks.py:278-284).
                    // ---- rigid / linear / sum: the instruction-lean form.  This kernel is bound by vector-instruction issue
                    // (SQ counters: the SIMDs issue ~88 % of the time, 435 VALU per query in the first form), so everything
                    // that can be decided once per neighbour is decided by the lane that stages it, not by the 16 lanes that
                    // consume it:  * a column that is not a real neighbour (shadow index, past the row) is staged as the
                    // shadow point (1e6,1e6,1e6) with row offset 0 -- its linear influence is exactly 0, no mask per step;
                    // * the row's element offset idx*ci is computed at staging;  * channel lanes past ci load row 0 and feed
                    // output columns that are never stored, no select;  * two steps share every arithmetic instruction
                    // (v_pk_* on float2): the staging layout puts (x_a,x_b,y_a,y_b) and (z_a,z_b,off_a,off_b) of the step
                    // pair (a, b) of a row group side by side, one ds_read_b128 each.
                    typedef float f2 __attribute__((ext_vector_type(2)));
                    float* nbf = reinterpret_cast<float*>(nb);       // [pair p = 0..7][kk = 0..3][8 floats]
                    float dn2 = 0.0f;
                    {
                        const bool real = idx >= 0 && (h0 + lane < h);
                        float sx = real ? px - qx : WS_SHADOW, sy = real ? py - qy : WS_SHADOW, sz = real ? pz - qz : WS_SHADOW;
                        if constexpr (MODE == 2) {
                            const bool incol = h0 + lane < h;
                            sx = incol ? px - qx : 3.0e18f; sy = incol ? py - qy : 3.0e18f; sz = incol ? pz - qz : 3.0e18f;
                        }
                        const unsigned off = real ? (unsigned)idx * (unsigned)ci : 0u;
                        const int sstep = lane >> 2, skk = lane & 3;  // this lane's neighbour is column 4 sstep + skk
                        float* dst = nbf + (((sstep >> 1) * 4 + skk) * 8) + (sstep & 1);
                        dst[0] = sx; dst[2] = sy; dst[4] = sz; dst[6] = __uint_as_float(off);
                        if constexpr (CUT) dn2 = real ? (sx * sx + sy * sy) + sz * sz : 3.4e38f;
                    }
                    int ncut = 64;
                    if constexpr (CUT) {
                        // sorted row: the columns inside the cutoff are a prefix of the chunk
                        ncut = __builtin_popcountll(__ballot(dn2 <= cut2));
                        if (ncut == 0 && (MODE == 0 || h0 > 0)) break;
                    }
                    wave_lds_order();
                    const int cols = min(min(64, h - h0), ncut);
                    const int steps = (cols + 3) >> 2;
                    const int npairs = (steps + 1) >> 1;
                    constexpr int GP = GS >= 2 ? GS / 2 : 1;         // step pairs whose loads are in flight together
                    const T* xlane = x + (chok ? ch : 0);
                    f2 wb2[2][GP];
                    float xb[2][2 * GP][NT];
                    auto load_pairs = [&](int gi, int slot) {
                        float4 va[GP], vb[GP];
#pragma unroll
                        for (int u = 0; u < GP; ++u) {
                            const float4* src = reinterpret_cast<const float4*>(nbf + ((gi * GP + u) * 4 + kk) * 8);
                            va[u] = src[0];
                            vb[u] = src[1];
                        }
#pragma unroll
                        for (int u = 0; u < GP; ++u) {
                            RowLoad<NT, T>::ld(xlane + __float_as_uint(vb[u].z), xb[slot][2 * u]);
                            RowLoad<NT, T>::ld(xlane + __float_as_uint(vb[u].w), xb[slot][2 * u + 1]);
                        }
#pragma unroll
                        for (int u = 0; u < GP; ++u) {
                            const f2 dx = f2{va[u].x, va[u].y} - kx, dy = f2{va[u].z, va[u].w} - ky, dz = f2{vb[u].x, vb[u].y} - kz;
                            const f2 d2 = (dx * dx + dy * dy) + dz * dz;
                            const f2 sd = f2{__builtin_amdgcn_sqrtf(d2.x), __builtin_amdgcn_sqrtf(d2.y)};
                            const f2 w = 1.0f - sd * inv_extent;
                            wb2[slot][u] = f2{fmaxf(w.x, 0.0f), fmaxf(w.y, 0.0f)};
                            if constexpr (MODE == 2) {
                                wb2[slot][u] = wb2[slot][u] * kmod;
                                mind = fminf(mind, fminf(d2.x, d2.y));
                            }
                        }
                    };
                    auto comp_pairs = [&](int slot) {
#pragma unroll
                        for (int u = 0; u < GP; ++u) {
#pragma unroll
                            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb2[slot][u].x, xb[slot][2 * u][t], acc[t], 0, 0, 0);
#pragma unroll
                            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb2[slot][u].y, xb[slot][2 * u + 1][t], acc[t], 0, 0, 0);
                        }
                    };
                    const int ngroups = (npairs + GP - 1) / GP;
                    load_pairs(0, 0);
                    for (int gi = 0; gi < ngroups; gi += 2) {
                        if (gi + 1 < ngroups) load_pairs(gi + 1, 1);
                        comp_pairs(0);
                        if (gi + 1 < ngroups) {
                            if (gi + 2 < ngroups) load_pairs(gi + 2, 0);
                            comp_pairs(1);
                        }
                    }
                    if constexpr (CUT) {
                        if (ncut < 64) break;                         // the row left the cutoff inside this chunk
                        if constexpr (MODE == 2) {
                            if (h0 == 0) {
                                // from here on a neighbour matters only inside max(influence reach, what could still lower a minimum)
                                float m = fminf(mind, __shfl_xor(mind, 16, 64));
                                m = fminf(m, __shfl_xor(m, 32, 64));
                                const float reach = group_max(haskp ? __builtin_sqrtf(m) + rk : 0.0f);
                                const float R = fmaxf(rq, reach) * 1.0001f;
                                cut2 = R * R;
                            }
                        }
                    }
                    continue;
                }
                nb[lane] = make_float4(px - qx, py - qy, pz - qz, __int_as_float((h0 + lane < h) ? (idx >= 0 ? idx : -2) : -1));
                wave_lds_order();
                const int cols = min(64, h - h0);
                const int steps = (cols + 3) >> 2;
                float wb[2][GS];
                float xb[2][GS][NT];
                // three separate passes per group so that nothing waits between the independent accesses: all LDS
                // broadcasts, then all row loads (addresses from the broadcasts), then the weights (VALU under the loads);
                // selects instead of branches throughout (an exec-mask branch per step serialises the LDS round trips)
                auto load_group = [&](int gi, int slot) {
                    float4 nv[GS];
#pragma unroll
                    for (int u = 0; u < GS; ++u)
                        nv[u] = nb[min(4 * (gi * GS + u) + kk, 63)];
#pragma unroll
                    for (int u = 0; u < GS; ++u) {
                        const int s = gi * GS + u;
                        const int nidx = __float_as_int(nv[u].w);     // >= 0 real, -2 shadow column, -1 past the row
                        const bool live = nidx >= 0 && s < steps;
                        const unsigned row = live ? (unsigned)nidx : 0u;
                        const T* src = x + (size_t)(row * (unsigned)ci) + (chok ? ch : 0);
                        RowLoad<NT, T>::ld(src, xb[slot][u]);
                    }
#pragma unroll
                    for (int u = 0; u < GS; ++u) {
                        const int s = gi * GS + u;
                        const float4 n = nv[u];
                        const int nidx = __float_as_int(n.w);
                        const bool live = nidx >= 0 && s < steps;
                        // influence of this lane's kernel point on that neighbour
                        const float dx = n.x - kx, dy = n.y - ky, dz = n.z - kz;
                        const float d2 = (dx * dx + dy * dy) + dz * dz;
                        float w;
                        if (MODE == 0) {
                            w = fmaxf(1.0f - __builtin_amdgcn_sqrtf(d2) * inv_extent, 0.0f);
                        } else {
                            w = kp_weight(d2, g, inv_extent);
                            if (g.aggregation == WS_AGGREGATION_CLOSEST) {
                                // arg-min kernel point of this neighbour over the 16 lanes of the row group (first wins)
                                float bd = haskp ? d2 : 3.4e38f;
                                int bi = i;
#pragma unroll
                                for (int o = 1; o < 16; o <<= 1) {
                                    const float od = __shfl_xor(bd, o, 64);
                                    const int oi = __shfl_xor(bi, o, 64);
                                    const bool take = od < bd || (od == bd && oi < bi);
                                    bd = take ? od : bd;
                                    bi = take ? oi : bi;
                                }
                                w = bi != i ? 0.0f : w;
                            }
                            if (DEF) {
                                const unsigned long long m = __ballot(haskp && d2 < e2);
                                w = ((((unsigned)(m >> (16 * kk))) & 0xffffu) == 0u) ? 0.0f : w;     // no kernel point in range (blocks.py:301-325)
                                mind = (nidx != -1 && s < steps && haskp) ? fminf(mind, d2) : mind;
                            }
                        }
                        wb[slot][u] = (live && haskp) ? w : 0.0f;
                    }
                };
                auto comp_group = [&](int slot) {
#pragma unroll
                    for (int u = 0; u < GS; ++u)
#pragma unroll
                        for (int t = 0; t < NT; ++t)
                            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[slot][u], chok ? xb[slot][u][t] : 0.0f, acc[t], 0, 0, 0);
                };
                const int ngroups = (steps + GS - 1) / GS;
                load_group(0, 0);
                for (int gi = 0; gi < ngroups; gi += 2) {
                    if (gi + 1 < ngroups) load_group(gi + 1, 1);
                    comp_group(0);
                    if (gi + 1 < ngroups) {
                        if (gi + 2 < ngroups) load_group(gi + 2, 0);
                        comp_group(1);
                    }
                }
            }
            // D: lane (j = i, g = kk) holds kernel points 4 kk + r of its NT channels
            if constexpr (FUSE) {
                __shared__ float tile_all[16 * TILE_LD];
                __shared__ int tq_all[16];
                const int slot = 4 * (iter & 3) + wave;
                const bool valid = item < iend;
                if (lane == 0) tq_all[slot] = valid ? (int)q : -1;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = 4 * kk + r;
                    if (k < K) *reinterpret_cast<float2*>(&tile_all[slot * TILE_LD + k * 32 + 2 * i]) = make_float2(acc[0][r], acc[1][r]);
                }
                if ((iter & 3) == 3 || item + 4 >= iend_u) {
                    __shared__ float part_all[4 * 16 * 32];
                    __syncthreads();                              // the tile is complete
                    f32x4v o0 = f32x4v{0.f, 0.f, 0.f, 0.f}, o1 = o0;
                    const float* arow = &tile_all[i * TILE_LD + 120 * wave + kk];
#pragma unroll
                    for (int s_ = 0; s_ < 30; ++s_) {
                        const float a = arow[4 * s_];
                        o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wq[s_][0], o0, 0, 0, 0);
                        o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wq[s_][1], o1, 0, 0, 0);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {                 // D: lane (j, g) holds queries 4 g + r of output columns j, 16 + j
                        part_all[(wave * 16 + 4 * kk + r) * 32 + i] = o0[r];
                        part_all[(wave * 16 + 4 * kk + r) * 32 + 16 + i] = o1[r];
                    }
                    __syncthreads();
#pragma unroll
                    for (int e = threadIdx.x; e < 512; e += 256) {
                        const int qs = e >> 5, c = e & 31;
                        const int qq = tq_all[qs];
                        float v = (part_all[(0 * 16 + qs) * 32 + c] + part_all[(1 * 16 + qs) * 32 + c]) +
                                  (part_all[(2 * 16 + qs) * 32 + c] + part_all[(3 * 16 + qs) * 32 + c]);
                        if (fz.bias) v += fz.bias[c];
                        if (fz.act) v = v > 0.0f ? v : v * fz.slope;
                        // slots this tile did not fill (a short last tile) keep the index of an older query: masked by the count
                        const bool filled = qs < 4 * ((iter & 3) + 1);
                        if (qq >= 0 && filled) fz.out[(int64_t)qq * 32 + c] = v;
                    }
                    __syncthreads();                              // tile and partials are free again
                }
                ++iter;
            } else if (chok) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = 4 * kk + r;
                    if (k < K) {
                        float v[NT];
#pragma unroll
                        for (int t = 0; t < NT; ++t) v[t] = acc[t][r];
                        if (MODE != 0 && modulations) {
                            const float md = modulations[q * K + k];
#pragma unroll
                            for (int t = 0; t < NT; ++t) v[t] *= md;
                        }
                        RowLoad<NT, T>::st(wf + (q * K + k) * ci + ch, v);
                    }
                }
            }
        }
        if (DEF && min_d2) {
            mind = fminf(mind, __shfl_xor(mind, 16, 64));
            mind = fminf(mind, __shfl_xor(mind, 32, 64));
            if (kk == 0 && haskp) min_d2[q * K + i] = mind;
        }
        // rotate; the checks / selects on the prefetched values happen here, one item after their loads were issued
        p0x = idx1 >= 0 ? p1x : WS_SHADOW; p0y = idx1 >= 0 ? p1y : WS_SHADOW; p0z = idx1 >= 0 ? p1z : WS_SHADOW;
        idx0 = idx1;
        idx1 = chk(raw2);
        qv0 = qv1; qv1 = qv2; qv2 = qv3;
        qx = q1x; qy = q1y; qz = q1z;
        q1x = q2x; q1y = q2y; q1z = q2z;
    }
}

}  // namespace

namespace kpconv {

// kpconv_gather_fwd_mfma_kernel for ws_kpconv_gather_fwd* (MODE 0 / 1) and ws_kpconv_gather_fwd_def (MODE 2).  MODE 0 is rigid and
// MODE 2 deformable, only MODE 1 takes either; CUT exists for MODE 0 and 2; VECROW = false stays uninstantiated.
void launch_fwd_mfma(const GatherPlan& p, void* stream, const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int64_t* inds,
                     int32_t h, const void* x, int32_t ci, const float* kernel_points, const float* deformed_kp, const float* modulations,
                     const GeomParams& g, void* wf, float* min_d2, const int32_t* order)
{
    dispatch([&](auto bf, auto nt, auto mode, auto def, auto cut, auto kn) {
        using T = Row<bf.value>;
        if constexpr ((mode.value == 1 ? !cut.value : def.value == (mode.value == 2)) && (kn.value == 15 || (!bf.value && mode.value != 2)))
            kpconv_gather_fwd_mfma_kernel<nt.value, mode.value, def.value != 0, true, T, 0, cut.value != 0, false, kn.value>
                <<<p.grid, 256, 0, (hipStream_t)stream>>>(
                q_pts, nq, s_pts, ns, inds, h, (const T*)x, ci, kernel_points, deformed_kp, modulations, g, (T*)wf, min_d2, order);
    }, Flag{p.bf16}, Pick<1, 2, 4, 8, 16>{p.n}, Pick<0, 1, 2>{p.mode}, Flag{p.def}, Flag{p.cut}, Pick<WS_KP_SIZES>{p.k});
}

// kpconv_gather_fwd_kernel for ws_kpconv_gather_fwd* on the 3..4-channel input layer: float4 rows with one lane group, other rows in
// 4-byte pieces; bf16 rows are VEC only, MODE 0 is rigid
void launch_fwd_pool(const GatherPlan& p, void* stream, const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int64_t* inds,
                     int32_t h, const void* x, int32_t ci, const float* kernel_points, const float* deformed_kp, const float* modulations,
                     const GeomParams& g, void* wf, float* min_d2, const int32_t* order)
{
    dispatch([&](auto bf, auto vec, auto mode, auto def, auto kn) {
        using T = Row<bf.value>;
        if constexpr ((!bf.value || vec.value) && (mode.value == 1 || !def.value) && (kn.value == 15 || !bf.value))
            kpconv_gather_fwd_kernel<kn.value, vec.value ? 1 : 4, mode.value, def.value != 0, vec.value != 0, vec.value ? 4 : 1, T>
                <<<p.grid, 256, 0, (hipStream_t)stream>>>(
                q_pts, nq, s_pts, ns, inds, h, (const T*)x, ci, kernel_points, deformed_kp, modulations, g, (T*)wf, min_d2, order);
    }, Flag{p.bf16}, Flag{p.vec}, Pick<0, 1>{p.mode}, Flag{p.def}, Pick<WS_KP_SIZES>{p.k});
}

// kpconv_gather_fwd_mfma_kernel<..., FUSE> for ws_kpconv_layer_fwd_fused: rigid / linear / sum, 32 -> 32 f32 channels
void launch_fwd_fused(void* stream, const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int64_t* inds, int32_t h,
                      const float* x, int32_t ci, const float* kernel_points, const GeomParams& g, const int32_t* order, const FuseArgs& fz)
{
    kpconv_gather_fwd_mfma_kernel<2, 0, false, true, float, WS_FUSE_GS, false, true><<<ws_grid(nq, 4), 256, 0, (hipStream_t)stream>>>(
        q_pts, nq, s_pts, ns, inds, h, x, ci, kernel_points, nullptr, nullptr, g, nullptr, nullptr, order, fz);
}

}  // namespace kpconv
