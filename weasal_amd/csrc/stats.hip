// weasal_amd/csrc/stats.hip -- what the training loop logs per step, kept on the device.
//
//   ws_step_stats   utils/trainer_PseudoLabel.py:209,244-253 (trainer_WeakLabel.py:208,243-252): the log line of a step holds
//                   net.output_loss, net.reg_loss (the weak-label trainer: the gradient norm) and KPFCNN.accuracy
//                   (models/architectures.py:386-399, :786-799: #{argmax_c logits[i, :] == target_i} / N over ALL rows).  The reference
//                   reads each of them back with .item() every step; here they go into one 16-byte record of a ring in device
//                   memory that the host lands once per epoch (weasal_amd/loop.py: StepLog).
// A thread owns one row (C <= 64 floats, as in loss.hip); the hits of a wave are one ballot + popcount per trip, the four
// wave counts meet in LDS and ONE integer atomic per workgroup adds them to the record: integers, so the sum does not depend
// on the order and the record is run-to-run identical.  The record is zeroed (and its three floats copied) by a one-thread
// launch in front of the count on the same stream.
#include "ws_common.h"

namespace {

// class position of a raw label, exactly ce_target of loss.hip (the mapping of ops.cross_entropy)
__device__ __forceinline__ int stats_target(const int64_t* __restrict__ labels, int64_t i, const int64_t* __restrict__ lut, int lut_n,
                                            int c)
{
    int64_t t = labels[i];
    if (lut) t = lut[(t >= 0 && t < lut_n - 1) ? t : lut_n - 1];
    return (t >= 0 && t < c) ? (int)t : -1;
}

__global__ void step_record_kernel(const float* __restrict__ out_loss, const float* __restrict__ reg_loss,
                                   const float* __restrict__ extra, ws_step_record* __restrict__ rec)
{
    rec->out_loss = out_loss ? out_loss[0] : 0.0f;
    rec->reg_loss = reg_loss ? reg_loss[0] : 0.0f;
    rec->extra = extra ? extra[0] : 0.0f;
    rec->correct = 0;
}

__global__ __launch_bounds__(256) void step_correct_kernel(const float* __restrict__ logits, int64_t n, int c, int64_t ldl,
                                                           const int64_t* __restrict__ labels, const int64_t* __restrict__ lut,
                                                           int lut_n, int32_t* __restrict__ correct)
{
    __shared__ int red[4];
    int hits = 0;                                         // of this wave: the same number in all its lanes
    // every lane of a workgroup makes the same number of trips, so the ballot sees whole waves
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {
        const int64_t i = base + threadIdx.x;
        bool hit = false;
        if (i < n) {
            const int t = stats_target(labels, i, lut, lut_n, c);
            const float* x = logits + i * ldl;
            // torch.argmax: the first maximum; a NaN is larger than every number and the first NaN stays
            float best = x[0];
            int at = 0;
            for (int j = 1; j < c; ++j) {
                const float v = x[j];
                if (v > best || (v != v && best == best)) { best = v; at = j; }
            }
            hit = (at == t);                              // ignored rows (t = -1) never hit
        }
        hits += __popcll(__ballot(hit));
    }
    if (ws_lane() == 0) red[threadIdx.x >> 6] = hits;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int sum = (red[0] + red[1]) + (red[2] + red[3]);
        if (sum) atomicAdd(correct, sum);
    }
}

}  // namespace

extern "C" int ws_step_stats(const float* logits, int64_t n, int32_t c, int64_t ldl, const int64_t* labels, const int64_t* lut,
                             int32_t lut_n, const float* out_loss, const float* reg_loss, const float* extra, ws_step_record* ring,
                             int64_t cap, int64_t row, void* stream)
{
    WS_REQUIRE(n >= 0 && n <= 0x7fffffffll && c >= 1 && c <= WS_STEP_STATS_MAX_C && ldl >= c,
               "bad sizes n=%lld c=%d (c <= %d, n < 2^31: the count is an int32)", (long long)n, c, WS_STEP_STATS_MAX_C);
    WS_REQUIRE(ring && cap >= 1 && row >= 0 && row < cap, "row %lld outside the ring of %lld records", (long long)row, (long long)cap);
    WS_REQUIRE(n == 0 || (logits && labels), "NULL argument");
    WS_REQUIRE(!lut || lut_n >= 2, "the label table needs at least one value and the spare entry");
    hipStream_t st = (hipStream_t)stream;
    step_record_kernel<<<1, 1, 0, st>>>(out_loss, reg_loss, extra, ring + row);
    WS_LAUNCH_CHECK();
    if (n == 0) return WS_OK;
    step_correct_kernel<<<ws_grid(n, 256, WS_STEP_STATS_BLOCKS), 256, 0, st>>>(logits, n, c, ldl, labels, lut, lut_n,
                                                                             &ring[row].correct);
    WS_LAUNCH_CHECK();
    return WS_OK;
}
