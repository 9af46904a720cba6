// weasal_amd/csrc/refine.hip -- stage 2 of the method, pseudo-label refinement (pseudoLabel_refinement.py), on the votes
// resident in HBM: nothing of size N leaves the device.
//
//   ws_weak_mask      :63-68   weak = ones[N, C]; weak[idx_a] *= lb_a for every anchor a.  A 0/1 row is C bits and the product
//                              of rows is their AND: one uint32 per point, bit k set while class k survives.  AND is
//                              commutative and idempotent, so the atomics give the same words in any order and a duplicate
//                              index (inside a list or through a repeated anchor) applies once, like the fancy-index *=.
//   ws_refine_labels  :123-151 per point i, row r = proj[i] of the votes (:123-125; the weak labels are NOT projected):
//                              empty = max_k(probs[r, k] * weak[i, k]) < 0.01 * threshold (:137), label = empty ? no_label :
//                              preds[r] (:143-145), counts[label] += 1 by value for label in [0, n_counts) (:148-151).
// Every step is exact: a product with 0 or 1, a float32 widened to float64 against the host's double, integer counts.
// Index lists come from files the caller read: an entry outside its range is skipped, never dereferenced, and counted
// in status[WS_REFINE_BAD_*].
#include "ws_common.h"

namespace {

typedef unsigned long long u64;

constexpr int RF_ROWS = 256;              // points per workgroup tile (one per lane)
constexpr int RF_TILES_PER_BLOCK = 4;     // tiles a workgroup walks before it flushes its histogram, when there are enough
constexpr int RF_MAX_COUNTS = 4096;       // bins of the LDS histogram

__device__ __forceinline__ void status_add(int64_t* status, int which)
{
    atomicAdd((u64*)status + which, 1ull);
}

__global__ __launch_bounds__(256) void weak_mask_init_kernel(uint32_t* __restrict__ mask, int64_t n, uint32_t full)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) mask[i] = full;
}

// blockIdx.y strides over the selected rows, blockIdx.x * 256 + lane over the entries of a row (gridDim.x is sized from
// the mean row length, so that a typical anchor is one pass and a long one is shared by gridDim.x workgroups)
__global__ __launch_bounds__(256) void weak_mask_and_kernel(uint32_t* __restrict__ mask, int64_t n,
                                                            const int64_t* __restrict__ anchor_ptr,
                                                            const int64_t* __restrict__ anchor_idx, int64_t nnz,
                                                            const uint32_t* __restrict__ anchor_bits, int64_t na,
                                                            const int64_t* __restrict__ anchor_sel, int64_t n_sel,
                                                            int64_t* __restrict__ status)
{
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t s = blockIdx.y; s < n_sel; s += gridDim.y) {
        const int64_t a = anchor_sel ? anchor_sel[s] : s;
        if (a < 0 || a >= na) {
            if (blockIdx.x == 0 && threadIdx.x == 0) status_add(status, WS_REFINE_BAD_ANCHOR_SEL);
            continue;
        }
        int64_t beg = anchor_ptr[a], end = anchor_ptr[a + 1];
        if (beg < 0) beg = 0;
        if (end > nnz) end = nnz;
        const uint32_t bits = anchor_bits[a];
        for (int64_t e = beg + (int64_t)blockIdx.x * 256 + threadIdx.x; e < end; e += step) {
            const int64_t i = anchor_idx[e];
            if (i < 0 || i >= n) { status_add(status, WS_REFINE_BAD_ANCHOR_IDX); continue; }
            atomicAnd(&mask[i], bits);                         // result unused: the return-less form
        }
    }
}

// One point per lane.  Without a projection the rows of a tile are consecutive and are staged in LDS with coalesced loads
// (a row is c * 4 bytes, 36 for nine classes: neither 16-byte aligned nor a line per lane), row stride c | 1 so that the
// 64 lanes of a wave fall on different banks; with one, every lane reads its own row where it lies.
// LDS: [RF_ROWS * (c | 1)] floats (identity only), then n_counts histogram words.
__global__ __launch_bounds__(RF_ROWS) void refine_labels_kernel(const float* __restrict__ probs, const int32_t* __restrict__ preds,
                                                                int64_t m, int c, const uint32_t* __restrict__ mask,
                                                                const int32_t* __restrict__ proj, int64_t n, double thr,
                                                                int32_t no_label, int32_t* __restrict__ labels,
                                                                int64_t* __restrict__ counts, int n_counts,
                                                                int64_t* __restrict__ status)
{
    extern __shared__ float lds[];
    const int ld = c | 1;
    float* tile = lds;
    unsigned* hist = (unsigned*)(lds + (proj ? 0 : RF_ROWS * ld));
    for (int b = threadIdx.x; b < n_counts; b += RF_ROWS) hist[b] = 0u;
    __syncthreads();
    const int64_t tiles = (n + RF_ROWS - 1) / RF_ROWS;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {          // (the trip count is the same for the whole workgroup)
        const int64_t r0 = t * RF_ROWS;
        const int rows = (int)(n - r0 < RF_ROWS ? n - r0 : RF_ROWS);
        const int64_t i = r0 + threadIdx.x;
        const float* p = nullptr;
        int64_t row = -1;
        if (!proj) {
            const float* src = probs + r0 * c;                         // rows r0 .. r0 + rows < n <= m (checked by the host)
            for (int e = threadIdx.x; e < rows * c; e += RF_ROWS) tile[(e / c) * ld + (e % c)] = src[e];
            __syncthreads();
            if ((int)threadIdx.x < rows) { row = i; p = tile + threadIdx.x * ld; }
        } else if ((int)threadIdx.x < rows) {
            row = proj[i];
            if (row < 0 || row >= m) { row = -1; status_add(status, WS_REFINE_BAD_PROJ); }
            else p = probs + row * c;
        }
        if ((int)threadIdx.x < rows) {
            int32_t label = no_label;
            if (row >= 0) {
                const uint32_t bits = mask[i];
                float mx = 0.0f;
                for (int k = 0; k < c; ++k) {
                    const float v = (bits >> k & 1u) ? p[k] : 0.0f;    // probs * weak
                    if (k == 0 || v > mx || v != v) mx = v;            // np.max: a NaN stays
                }
                if (!((double)mx < thr)) label = preds[row];
                if (label >= 0 && label < n_counts) atomicAdd(&hist[label], 1u);
            }
            labels[i] = label;
        }
        if (!proj) __syncthreads();                                    // the tile is overwritten by the next pass
    }
    __syncthreads();
    for (int b = threadIdx.x; b < n_counts; b += RF_ROWS)
        if (hist[b]) atomicAdd((u64*)counts + b, (u64)hist[b]);
}

}  // namespace

extern "C" {

int ws_weak_mask(uint32_t* mask, int64_t n, int32_t c, const int64_t* anchor_ptr, const int64_t* anchor_idx, int64_t nnz,
                 const uint32_t* anchor_bits, int64_t n_anchors, const int64_t* anchor_sel, int64_t n_sel, int64_t* status,
                 void* stream)
{
    WS_REQUIRE(n >= 0 && nnz >= 0 && n_anchors >= 0 && n_sel >= 0 && c >= 1, "bad sizes n=%lld nnz=%lld anchors=%lld sel=%lld c=%d",
               (long long)n, (long long)nnz, (long long)n_anchors, (long long)n_sel, c);
    if (c > 32) return ws_fail(WS_ERR_UNSUPPORTED, "ws_weak_mask: c=%d classes (at most 32)", c);
    if (n == 0) return WS_OK;
    const int64_t rows = anchor_sel ? n_sel : n_anchors;
    WS_REQUIRE(mask && status && (n_sel == 0 || anchor_sel) && (rows == 0 || (anchor_ptr && anchor_bits)) &&
               (nnz == 0 || rows == 0 || anchor_idx), "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const uint32_t full = c == 32 ? 0xFFFFFFFFu : (1u << c) - 1u;
    weak_mask_init_kernel<<<ws_grid(n, 256 * 8, 2048), 256, 0, st>>>(mask, n, full);
    WS_LAUNCH_CHECK();
    if (rows == 0) return WS_OK;
    int64_t gx = n_anchors > 0 ? ws_ceil_div(ws_ceil_div(nnz, n_anchors), 256) : 1;
    gx = gx < 1 ? 1 : gx > 64 ? 64 : gx;
    int64_t gy = 4096 / gx;
    gy = rows < gy ? rows : gy;
    weak_mask_and_kernel<<<dim3((unsigned)gx, (unsigned)gy), 256, 0, st>>>(mask, n, anchor_ptr, anchor_idx, nnz, anchor_bits, n_anchors,
                                                                       anchor_sel, rows, status);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_refine_labels(const float* probs, const int32_t* preds, int64_t m, int32_t c, const uint32_t* mask, const int32_t* proj,
                     int64_t n, double thr, int32_t no_label, int32_t* labels, int64_t* counts, int32_t n_counts, int64_t* status,
                     void* stream)
{
    WS_REQUIRE(n >= 0 && m >= 0 && c >= 1 && n_counts >= 0, "bad sizes n=%lld m=%lld c=%d n_counts=%d", (long long)n, (long long)m, c,
               n_counts);
    if (c > 32) return ws_fail(WS_ERR_UNSUPPORTED, "ws_refine_labels: c=%d classes (at most 32)", c);
    if (n_counts > RF_MAX_COUNTS)
        return ws_fail(WS_ERR_UNSUPPORTED, "ws_refine_labels: n_counts=%d bins (at most %d)", n_counts, RF_MAX_COUNTS);
    if (n == 0) return WS_OK;
    WS_REQUIRE(mask && labels && status && (n_counts == 0 || counts) && (m == 0 || (probs && preds)), "NULL argument");
    WS_REQUIRE(proj || m >= n, "without a projection the votes need a row per point: m=%lld < n=%lld", (long long)m, (long long)n);
    const int64_t tiles = ws_ceil_div(n, RF_ROWS);
    const size_t lds = sizeof(float) * (proj ? 0 : RF_ROWS * (c | 1)) + sizeof(unsigned) * n_counts;
    refine_labels_kernel<<<ws_grid(tiles, RF_TILES_PER_BLOCK, 2048), RF_ROWS, lds, (hipStream_t)stream>>>(
        probs, preds, m, c, mask, proj, n, thr, no_label, labels, counts, n_counts, status);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

}  // extern "C"
