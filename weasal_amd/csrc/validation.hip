// weasal_amd/csrc/validation.hip -- the per-epoch validation pass of the training loop, one launch per batch.
//
//   ws_validation_update  utils/trainer_PseudoLabel.py:368-407 : softmax of the logits and the exponential smoothing of the
//                         per-cloud validation votes at every sphere's input indices, sphere after sphere;
//                         :423-436 + utils/metrics.py:35-110 : arg-max of every row's softmax against its label, counted
//                         in the epoch's confusion matrix
//
// The reference updates the votes one sphere at a time, so a point that several spheres of a batch list ends as the chain
// s*(s*p + (1-s)*a1) + (1-s)*a2 in sphere order.  One launch over all rows reproduces it by ownership: of the rows that
// list a point, the one in the LAST sphere owns it; it reads the vote row once, applies every member's update in ascending
// sphere order (the softmax of an earlier member is recomputed from its logits) and writes the row once.  Every other row
// leaves the votes alone.  One writer per point: no race, no float atomic, the same bits on every run.  The other members
// are found by binary search in the ascending input_inds slice of the spheres the caller's mask names.
// The float32 expressions are those of vote_update_kernel (tester.hip): max, expf, sum, smooth*p + (1-smooth)*q.
#include "ws_common.h"

namespace {

constexpr int VAL_MAX = WS_PYRAMID_MAX_BATCH;
struct ValTable {
    int32_t off[VAL_MAX];
    int32_t len[VAL_MAX];
    int32_t cloud[VAL_MAX];
    uint64_t mask[VAL_MAX];       // the other spheres of the same cloud that may share points with this one
};

// test_radius_ratio mask of tester.hip: sum(points^2) < r2 in f32; no mask when r2 == 0
__device__ __forceinline__ bool val_inside(const float* __restrict__ points, float r2, int64_t i)
{
    if (!(r2 > 0.0f)) return true;
    const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
    return ((x * x + y * y) + z * z) < r2;
}

// position of v in the ascending slice a[0, len), -1 when absent; every read stays inside the slice whatever it holds
__device__ __forceinline__ int val_find(const int64_t* __restrict__ a, int len, int64_t v)
{
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return (lo < len && a[lo] == v) ? lo : -1;
}

template <int CM>
__device__ __forceinline__ void val_apply(float (&acc)[CM], const float* __restrict__ l, int c, float smooth)
{
    float m = l[0];
    for (int k = 1; k < c; ++k) m = fmaxf(m, l[k]);
    float s = 0.0f;
    for (int k = 0; k < c; ++k) s += expf(l[k] - m);
#pragma unroll
    for (int k = 0; k < CM; ++k)
        if (k < c) acc[k] = smooth * acc[k] + (1.0f - smooth) * (expf(l[k] - m) / s);
}

// One row per lane.  CM: the vote row lives in CM registers (c <= CM).
template <int CM>
__global__ __launch_bounds__(256) void validation_kernel(const float* __restrict__ logits, int64_t n, int c, int64_t ld,
                                                         const int64_t* __restrict__ inds, const int64_t* __restrict__ labels,
                                                         const float* __restrict__ points, float r2, ValTable t, int nb,
                                                         float* const* __restrict__ votes, const int64_t* __restrict__ cloud_rows,
                                                         float smooth, const int32_t* __restrict__ true_row, int n_true,
                                                         const int32_t* __restrict__ pred_row, int nc,
                                                         long long* __restrict__ confusion, long long* __restrict__ status)
{
    __shared__ ValTable s;
    __shared__ int hist[64 * 64];
    if (threadIdx.x < VAL_MAX) {
        const int e = threadIdx.x;
        const bool on = e < nb;
        s.off[e] = on ? t.off[e] : 0;
        s.len[e] = on ? t.len[e] : 0;
        s.cloud[e] = on ? t.cloud[e] : 0;
        s.mask[e] = on ? t.mask[e] : 0ull;
    }
    if (labels)
        for (int e = threadIdx.x; e < nc * nc; e += 256) hist[e] = 0;
    __syncthreads();

    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int b = -1;
        for (int e = 0; e < nb; ++e)
            if (i >= s.off[e] && i < (int64_t)s.off[e] + s.len[e]) b = e;
        if (b < 0) continue;                                          // a row between two spheres belongs to nobody
        const int64_t idx = inds[i];
        if (i > s.off[b] && inds[i - 1] >= idx) atomicAdd((unsigned long long*)&status[WS_VAL_UNSORTED], 1ull);
        const float* l = logits + i * ld;

        if (labels) {                                                 // every row, whatever the mask and whoever owns it
            float m = l[0];
            for (int k = 1; k < c; ++k) m = fmaxf(m, l[k]);
            float sum = 0.0f;
            for (int k = 0; k < c; ++k) sum += expf(l[k] - m);
            int best = 0;
            float bv = expf(l[0] - m) / sum;
            for (int k = 1; k < c; ++k) {
                const float v = expf(l[k] - m) / sum;
                if (v > bv) { bv = v; best = k; }
            }
            const int64_t lab = labels[i];
            int tr = -1, pr = -1;
            if (lab >= 0 && lab < n_true) { tr = true_row[lab]; pr = pred_row[best]; }
            if (tr >= 0 && tr < nc && pr >= 0 && pr < nc) atomicAdd(&hist[tr * nc + pr], 1);
            else atomicAdd((unsigned long long*)&status[WS_VAL_BAD_LABEL], 1ull);
        }

        const int cl = s.cloud[b];
        if (idx < 0 || idx >= cloud_rows[cl]) {
            atomicAdd((unsigned long long*)&status[WS_VAL_BAD_INDEX], 1ull);
            continue;
        }
        if (!val_inside(points, r2, i)) continue;
        const uint64_t mask = s.mask[b];
        bool owner = true;
        for (uint64_t later = b == 63 ? 0ull : mask & (~0ull << (b + 1)); later; later &= later - 1) {
            const int b2 = __ffsll((long long)later) - 1;
            if (s.cloud[b2] != cl) continue;
            const int j = val_find(inds + s.off[b2], s.len[b2], idx);
            if (j >= 0 && val_inside(points, r2, (int64_t)s.off[b2] + j)) { owner = false; break; }
        }
        if (!owner) continue;

        float* p = votes[cl] + idx * c;
        float acc[CM];
#pragma unroll
        for (int k = 0; k < CM; ++k) acc[k] = k < c ? p[k] : 0.0f;
        for (uint64_t earlier = mask & ((1ull << b) - 1ull); earlier; earlier &= earlier - 1) {
            const int b2 = __ffsll((long long)earlier) - 1;
            if (s.cloud[b2] != cl) continue;
            const int j = val_find(inds + s.off[b2], s.len[b2], idx);
            if (j < 0) continue;
            const int64_t row = (int64_t)s.off[b2] + j;
            if (val_inside(points, r2, row)) val_apply<CM>(acc, logits + row * ld, c, smooth);
        }
        val_apply<CM>(acc, l, c, smooth);
#pragma unroll
        for (int k = 0; k < CM; ++k)
            if (k < c) p[k] = acc[k];
    }

    if (labels) {
        __syncthreads();
        for (int e = threadIdx.x; e < nc * nc; e += 256)
            if (hist[e]) atomicAdd((unsigned long long*)&confusion[e], (unsigned long long)hist[e]);
    }
}

}  // namespace

extern "C" {

int ws_validation_update(const float* logits, int64_t n, int32_t c, int64_t ld, const int64_t* input_inds, const int64_t* labels,
                         const float* points, float radius_mask, const int64_t* h_offsets, const int32_t* h_lens,
                         const int32_t* h_clouds, const uint64_t* h_overlap, int32_t nb, float* const* votes,
                         const int64_t* cloud_rows, int32_t n_clouds, float smooth, const int32_t* true_row, int32_t n_true,
                         const int32_t* pred_row, int32_t nc, int64_t* confusion, int64_t* status, void* stream)
{
    WS_REQUIRE(n >= 0 && c >= 1 && nb >= 1 && n_clouds >= 1, "bad sizes n=%lld c=%d nb=%d n_clouds=%d", (long long)n, c, nb, n_clouds);
    if (c > 64) return ws_fail(WS_ERR_UNSUPPORTED, "c=%d: at most 64 classes", c);
    if (nb > VAL_MAX) return ws_fail(WS_ERR_UNSUPPORTED, "nb=%d: at most %d spheres per batch", nb, VAL_MAX);
    WS_REQUIRE(ld >= c, "leading dimension %lld below c=%d", (long long)ld, c);
    if (n > 2147483647ll) return ws_fail(WS_ERR_UNSUPPORTED, "n=%lld: at most 2^31 - 1 rows per batch", (long long)n);
    if (labels) {
        WS_REQUIRE(nc >= 1 && n_true >= 1, "bad sizes nc=%d n_true=%d", nc, n_true);
        if (nc > 64) return ws_fail(WS_ERR_UNSUPPORTED, "nc=%d: at most 64 label values", nc);
    }
    if (n == 0) return WS_OK;
    WS_REQUIRE(logits && input_inds && h_offsets && h_lens && h_clouds && h_overlap && votes && cloud_rows && status, "NULL argument");
    WS_REQUIRE(radius_mask <= 0.0f || points, "NULL argument: a radius mask needs the points");
    WS_REQUIRE(!labels || (true_row && pred_row && confusion), "NULL argument: labels need true_row, pred_row and a confusion matrix");
    ValTable t;
    int64_t end = 0;
    for (int b = 0; b < nb; ++b) {
        WS_REQUIRE(h_lens[b] >= 0 && h_offsets[b] >= end && h_offsets[b] + h_lens[b] <= n,
                   "sphere %d: rows [%lld, %lld + %d) overlap the sphere before or leave [0, %lld)", b, (long long)h_offsets[b],
                   (long long)h_offsets[b], h_lens[b], (long long)n);
        WS_REQUIRE(h_clouds[b] >= 0 && h_clouds[b] < n_clouds, "sphere %d: cloud %d outside [0, %d)", b, h_clouds[b], n_clouds);
        WS_REQUIRE(nb == 64 || (h_overlap[b] >> nb) == 0, "sphere %d: the overlap mask names spheres beyond nb=%d", b, nb);
        end = h_offsets[b] + h_lens[b];
        t.off[b] = (int32_t)h_offsets[b];
        t.len[b] = h_lens[b];
        t.cloud[b] = h_clouds[b];
    }
    for (int b = 0; b < nb; ++b) {
        uint64_t m = 0;
        for (int b2 = 0; b2 < nb; ++b2) {
            const bool ab = (h_overlap[b] >> b2) & 1, ba = (h_overlap[b2] >> b) & 1;
            WS_REQUIRE(ab == ba, "the overlap masks of spheres %d and %d disagree", b, b2);
            if (ab && b2 != b && h_clouds[b2] == h_clouds[b]) m |= 1ull << b2;     // same cloud only; never itself
        }
        t.mask[b] = m;
    }
    const float r2 = radius_mask > 0.0f ? radius_mask * radius_mask : 0.0f;
    const int grid = ws_grid(n, 256, 1024);
    hipStream_t st = (hipStream_t)stream;
    if (c <= 16)
        validation_kernel<16><<<grid, 256, 0, st>>>(logits, n, c, ld, input_inds, labels, points, r2, t, nb, votes, cloud_rows, smooth,
                                                    true_row, n_true, pred_row, nc, (long long*)confusion, (long long*)status);
    else
        validation_kernel<64><<<grid, 256, 0, st>>>(logits, n, c, ld, input_inds, labels, points, r2, t, nb, votes, cloud_rows, smooth,
                                                    true_row, n_true, pred_row, nc, (long long*)confusion, (long long*)status);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

}  // extern "C"
