// weasal_amd/csrc/testrun.hip -- the end of a test run, one launch per cloud (weasal_amd/testrun.py).
//
//   ws_test_outputs  utils/tester_PseudoLabel.py:277 : the votes re-projected on the full-resolution points;
//                    :297-300 : a zero column per ignored label (np.insert), the row the probs/ files hold;
//                    :303 : label_values[np.argmax(row)]; :345-348 : the error map; :307 + utils/metrics.py:35-110 : the
//                    confusion against the full-resolution labels.  proj == NULL is the sub-cloud form of :231-244.
//
// The vote rows are a random gather (sub-cloud rows lie in hash-map order), 4 * c bytes each; everything written is a
// stream.  A workgroup takes `rows` consecutive points at a time: lane t gathers the row of point base + t, lays the
// expanded row into an LDS tile [rows, c_all] and takes its first maximum there; then all lanes copy the tile, which is
// the contiguous span proj_probs[base * c_all, (base + cnt) * c_all), in float4 steps.  No value is computed, only moved
// and compared: the same bits on every run.  The confusion is a per-workgroup LDS histogram flushed with integer atomics.
#include "ws_common.h"

namespace {

constexpr int TEST_MAX_C = 64;
constexpr int TEST_GRID_CAP = 2048;            // workgroups; beyond it a workgroup strides over the tiles

__global__ __launch_bounds__(256) void test_outputs_kernel(const float* __restrict__ votes, int64_t n_sub, int c,
                                                           const int32_t* __restrict__ proj, int64_t m,
                                                           const int32_t* __restrict__ col_of,
                                                           const int32_t* __restrict__ label_values, int c_all,
                                                           const int32_t* __restrict__ targets,
                                                           const int32_t* __restrict__ true_row, int n_true,
                                                           float* __restrict__ proj_probs, int32_t* __restrict__ preds,
                                                           int8_t* __restrict__ error, long long* __restrict__ confusion,
                                                           long long* __restrict__ status, int rows, int vec)
{
    extern __shared__ float4 smem4[];
    float* tile = (float*)smem4;                               // [rows, c_all]; rows % 4 == 0: the next array stays aligned
    int* s_col = (int*)(tile + rows * c_all);                  // [TEST_MAX_C] position of vote column k in the expanded row
    int* s_val = s_col + TEST_MAX_C;                           // [TEST_MAX_C] label value of expanded position j
    int* hist = s_val + TEST_MAX_C;                            // [c_all, c_all]
    const int tid = threadIdx.x;
    if (tid < TEST_MAX_C) {
        s_col[tid] = tid < c ? col_of[tid] : -1;
        s_val[tid] = tid < c_all ? label_values[tid] : 0;
    }
    if (confusion)
        for (int e = tid; e < c_all * c_all; e += 256) hist[e] = 0;
    __syncthreads();

    const int64_t n_tiles = (m + rows - 1) / rows;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t base = t * rows;
        const int cnt = (int)(m - base < rows ? m - base : rows);
        if (tid < cnt) {
            const int64_t i = base + tid;
            float* e = tile + tid * c_all;
            for (int j = 0; j < c_all; ++j) e[j] = 0.0f;
            const int64_t p = proj ? (int64_t)proj[i] : i;
            const bool row_ok = p >= 0 && p < n_sub;
            if (row_ok) {
                const float* r = votes + p * c;
                for (int k = 0; k < c; ++k) {
                    const int col = s_col[k];
                    if ((unsigned)col < (unsigned)c_all) e[col] = r[k];
                }
            } else {
                atomicAdd((unsigned long long*)&status[WS_TEST_BAD_PROJ], 1ull);
            }
            int best = 0;                                      // np.argmax of the expanded row: the first maximum
            float bv = e[0];
            for (int j = 1; j < c_all; ++j) {
                const float v = e[j];
                if (v > bv) { bv = v; best = j; }
            }
            const int value = s_val[best];
            if (preds) preds[i] = value;
            if (targets) {
                const int tg = targets[i];
                if (error) error[i] = (int8_t)(value != tg);
                if (confusion) {
                    int tr = -1;
                    if (tg >= 0 && tg < n_true) tr = true_row[tg];
                    if ((unsigned)tr >= (unsigned)c_all) atomicAdd((unsigned long long*)&status[WS_TEST_BAD_TARGET], 1ull);
                    else if (row_ok) atomicAdd(&hist[tr * c_all + best], 1);
                }
            }
        }
        if (proj_probs) {
            __syncthreads();
            float* dst = proj_probs + base * c_all;
            const int total = cnt * c_all;
            const int n4 = vec ? total >> 2 : 0;               // base * c_all is a multiple of 4 elements: rows % 4 == 0
            for (int q = tid; q < n4; q += 256) ((float4*)dst)[q] = ((const float4*)tile)[q];
            for (int q = 4 * n4 + tid; q < total; q += 256) dst[q] = tile[q];
            __syncthreads();                                   // the next tile overwrites what is being read
        }
    }

    if (confusion) {
        __syncthreads();
        for (int e = tid; e < c_all * c_all; e += 256)
            if (hist[e]) atomicAdd((unsigned long long*)&confusion[e], (unsigned long long)hist[e]);
    }
}

}  // namespace

extern "C" {

// rows of a tile: 256 (one per lane) while tile + tables + histogram fit 64 KiB of LDS, else 128
static int test_outputs_rows(int c_all)
{
    const size_t fixed = sizeof(int) * (2 * TEST_MAX_C + (size_t)c_all * c_all);
    return sizeof(float) * 256 * (size_t)c_all + fixed <= 65536 ? 256 : 128;
}

int ws_test_outputs(const float* votes, int64_t n_sub, int32_t c, const int32_t* proj, int64_t m, const int32_t* col_of,
                    const int32_t* label_values, int32_t c_all, const int32_t* targets, const int32_t* true_row, int32_t n_true,
                    float* proj_probs, int32_t* preds, int8_t* error, int64_t* confusion, int64_t* status, void* stream)
{
    WS_REQUIRE(m >= 0 && n_sub >= 0 && c >= 1 && c_all >= 1 && n_true >= 0, "bad sizes m=%lld n_sub=%lld c=%d c_all=%d n_true=%d",
               (long long)m, (long long)n_sub, c, c_all, n_true);
    if (c_all > TEST_MAX_C) return ws_fail(WS_ERR_UNSUPPORTED, "c_all=%d: at most %d label values", c_all, TEST_MAX_C);
    if (c > c_all) return ws_fail(WS_ERR_UNSUPPORTED, "c=%d vote columns for c_all=%d label values", c, c_all);
    if (m == 0) return WS_OK;
    WS_REQUIRE(votes && col_of && label_values && status, "NULL argument");
    WS_REQUIRE(!error || targets, "NULL argument: the error map needs the targets");
    WS_REQUIRE(!confusion || (targets && true_row && n_true >= 1), "NULL argument: the confusion needs the targets and true_row");
    const int rows = test_outputs_rows(c_all);
    const size_t lds = sizeof(float) * rows * (size_t)c_all + sizeof(int) * (2 * TEST_MAX_C + (size_t)c_all * c_all);
    const int vec = ((uintptr_t)proj_probs & 15) == 0;
    test_outputs_kernel<<<ws_grid(m, rows, TEST_GRID_CAP), 256, lds, (hipStream_t)stream>>>(
        votes, n_sub, c, proj, m, col_of, label_values, c_all, targets, true_row, n_true, proj_probs, preds, error,
        (long long*)confusion, (long long*)status, rows, vec);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

}  // extern "C"
