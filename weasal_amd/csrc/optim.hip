// weasal_amd/csrc/optim.hip -- the parameter update of the training step in one pass over the parameters.
//
//   ws_sgd_step   utils/trainer_PseudoLabel.py:216-218 (torch.nn.utils.clip_grad_value_ then optimizer.step()) with the
//                 optimizer of :72-82 (torch.optim.SGD, momentum, weight decay, no dampening / Nesterov):
//                     g   = clamp(grad, -clip, clip)                  (clip > 0)
//                     g  += weight_decay * p                          (weight_decay != 0)
//                     buf = first ? g : momentum * buf + g            (momentum != 0)
//                     p  -= lr * buf
// The stock path is one clamp, and three to four `foreach` passes over ~230 tensors (0.36 ms and ~7 launches of
// multi_tensor_apply per DALES step); here every parameter element is read and written once: p, grad, buf in, p, buf out.
// A launch takes up to WS_SGD_MAX tensors as kernel arguments (pointer table + block prefix): no device-side table,
// no host-to-device copy, ~230 tensors = 3 launches.
//
//   ws_grad_norm        utils/trainer_WeakLabel.py:216 (torch.nn.utils.clip_grad_norm_): the total 2-norm of all gradient
//                       tensors and coef = min(1, max_norm / (total_norm + 1e-6)), both left in device memory.  Every
//                       workgroup writes the sum of squares of its SGD_CHUNK elements into a slot of its own; a finishing
//                       launch adds the slots in index order (64 contiguous runs, then the 64 run sums): no float atomic.
//   ws_sgd_step_scaled  ws_sgd_step with g = g * coef (read from that device word) in front of weight decay and momentum;
//                       the scaled gradient is written back (what clip_grad_norm_ leaves in p.grad).
#include "ws_common.h"

namespace {

constexpr int SGD_MAX = 96;            // tensors per launch: 96 x (3 pointers + size + block prefix) = 3.5 KB of kernel arguments
constexpr int SGD_CHUNK = 4096;        // elements per workgroup

struct SgdArgs {
    float* p[SGD_MAX];
    const float* g[SGD_MAX];
    float* buf[SGD_MAX];
    int n[SGD_MAX];
    int first_block[SGD_MAX + 1];
    int count;
};

__device__ __forceinline__ float sgd_one(float p, float g, float& b, float lr, float momentum, float wd, float clip, int first)
{
    if (clip > 0.0f) g = fminf(fmaxf(g, -clip), clip);
    if (wd != 0.0f) g = __fadd_rn(g, __fmul_rn(wd, p));
    if (momentum != 0.0f) {
        b = first ? g : __fadd_rn(__fmul_rn(b, momentum), g);
        g = b;
    }
    return __fadd_rn(p, __fmul_rn(-lr, g));
}

// SCALED: the gradient is multiplied by the device word `coef` first and written back (skipped when coef is exactly 1:
// the product is the gradient itself)
template <bool SCALED>
__global__ __launch_bounds__(256) void sgd_step_kernel(const SgdArgs a, float lr, float momentum, float wd, float clip, int first,
                                                       const float* __restrict__ coef)
{
    // tensor of this workgroup: the prefix is ascending, <= 96 entries -> binary search on scalars
    int lo = 0, hi = a.count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.first_block[mid] <= (int)blockIdx.x) lo = mid; else hi = mid;
    }
    float* __restrict__ p = a.p[lo];
    const float* __restrict__ g = a.g[lo];
    float* __restrict__ gw = const_cast<float*>(a.g[lo]);       // (SCALED only)
    float* __restrict__ buf = a.buf[lo];
    const float cf = SCALED ? coef[0] : 1.0f;
    const bool put = SCALED && cf != 1.0f;
    const int n = a.n[lo];
    const int base = ((int)blockIdx.x - a.first_block[lo]) * SGD_CHUNK;
    const int end = base + SGD_CHUNK < n ? base + SGD_CHUNK : n;
    const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(buf)) & 15u) == 0;
    int i = base + 4 * threadIdx.x;
    if (vec) {
        for (; i + 3 < end; i += 1024) {
            float4 pv = *reinterpret_cast<const float4*>(p + i);
            float4 gv = *reinterpret_cast<const float4*>(g + i);
            if (SCALED) {
                gv.x = __fmul_rn(gv.x, cf); gv.y = __fmul_rn(gv.y, cf); gv.z = __fmul_rn(gv.z, cf); gv.w = __fmul_rn(gv.w, cf);
                if (put) *reinterpret_cast<float4*>(gw + i) = gv;
            }
            float4 bv = (buf && !first) ? *reinterpret_cast<const float4*>(buf + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            pv.x = sgd_one(pv.x, gv.x, bv.x, lr, momentum, wd, clip, first);
            pv.y = sgd_one(pv.y, gv.y, bv.y, lr, momentum, wd, clip, first);
            pv.z = sgd_one(pv.z, gv.z, bv.z, lr, momentum, wd, clip, first);
            pv.w = sgd_one(pv.w, gv.w, bv.w, lr, momentum, wd, clip, first);
            *reinterpret_cast<float4*>(p + i) = pv;
            if (buf) *reinterpret_cast<float4*>(buf + i) = bv;
        }
        // the (at most 3) elements past the last whole quad of the tensor: the thread whose quad straddles `end`
        if (i < end) {
            for (int e = i; e < end; ++e) {
                float b = (buf && !first) ? buf[e] : 0.0f;
                float ge = g[e];
                if (SCALED) { ge = __fmul_rn(ge, cf); if (put) gw[e] = ge; }
                p[e] = sgd_one(p[e], ge, b, lr, momentum, wd, clip, first);
                if (buf) buf[e] = b;
            }
        }
    } else {
        for (int e = base + threadIdx.x; e < end; e += 256) {
            float b = (buf && !first) ? buf[e] : 0.0f;
            float ge = g[e];
            if (SCALED) { ge = __fmul_rn(ge, cf); if (put) gw[e] = ge; }
            p[e] = sgd_one(p[e], ge, b, lr, momentum, wd, clip, first);
            if (buf) buf[e] = b;
        }
    }
}

struct NormArgs {
    const float* g[SGD_MAX];
    int n[SGD_MAX];
    int first_block[SGD_MAX + 1];
    int count;
};

// slot[slot0 + workgroup] = sum of the squares of the workgroup's SGD_CHUNK elements: thread t adds its elements in index
// order, the lanes of a wave fold by xor-shuffles, the four wave sums are added in wave order
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const NormArgs a, float* __restrict__ slots, int slot0)
{
    __shared__ float wsum[4];
    int lo = 0, hi = a.count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.first_block[mid] <= (int)blockIdx.x) lo = mid; else hi = mid;
    }
    const float* __restrict__ g = a.g[lo];
    const int n = a.n[lo];
    const int base = ((int)blockIdx.x - a.first_block[lo]) * SGD_CHUNK;
    const int end = base + SGD_CHUNK < n ? base + SGD_CHUNK : n;
    float acc = 0.0f;
    int i = base + 4 * threadIdx.x;
    if ((reinterpret_cast<uintptr_t>(g) & 15u) == 0) {
        for (; i + 3 < end; i += 1024) {
            const float4 v = *reinterpret_cast<const float4*>(g + i);
            acc = __fmaf_rn(v.x, v.x, acc); acc = __fmaf_rn(v.y, v.y, acc); acc = __fmaf_rn(v.z, v.z, acc); acc = __fmaf_rn(v.w, v.w, acc);
        }
        if (i < end)
            for (int e = i; e < end; ++e) acc = __fmaf_rn(g[e], g[e], acc);
    } else {
        for (int e = base + threadIdx.x; e < end; e += 256) acc = __fmaf_rn(g[e], g[e], acc);
    }
    acc = ws_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) slots[slot0 + blockIdx.x] = __fadd_rn(__fadd_rn(__fadd_rn(wsum[0], wsum[1]), wsum[2]), wsum[3]);
}

// one wave: lane l adds the slots of its contiguous run in index order, lane 0 adds the 64 run sums in lane order
__global__ __launch_bounds__(64) void grad_norm_finish_kernel(const float* __restrict__ slots, int nslots, float max_norm,
                                                              float* __restrict__ out)
{
    __shared__ float run[64];
    const int per = (nslots + 63) / 64;
    const int beg = threadIdx.x * per, end = beg + per < nslots ? beg + per : nslots;
    float acc = 0.0f;
    for (int i = beg; i < end; ++i) acc = __fadd_rn(acc, slots[i]);
    run[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = run[0];
        for (int l = 1; l < 64; ++l) s = __fadd_rn(s, run[l]);
        const float total = sqrtf(s);
        out[0] = total;
        out[1] = fminf(1.0f, __fdiv_rn(max_norm, __fadd_rn(total, 1e-6f)));
    }
}

// the tensor table of one launch from the host arrays, starting at tensor t (advanced); empty tensors are passed over
template <typename Args, typename Fill>
int fill_table(Args& a, const int64_t* h_sizes, int32_t count, int& t, int& blocks, Fill fill)
{
    a.count = 0;
    blocks = 0;
    while (t < count && a.count < SGD_MAX) {
        const int64_t n = h_sizes[t];
        WS_REQUIRE(n >= 0 && n < (1ll << 31) - SGD_CHUNK, "tensor %d too large (%lld elements)", t, (long long)n);
        if (n > 0) {
            const int j = a.count;
            if (int rc = fill(j, t)) return rc;
            a.count = j + 1;
            a.n[j] = (int)n;
            a.first_block[j] = blocks;
            blocks += (int)ws_ceil_div(n, SGD_CHUNK);
        }
        ++t;
    }
    a.first_block[a.count] = blocks;
    return WS_OK;
}

}  // namespace

extern "C" {

int64_t ws_grad_norm_slots(const int64_t* h_sizes, int32_t count)
{
    int64_t slots = 0;
    for (int t = 0; h_sizes && t < count; ++t) slots += h_sizes[t] > 0 ? ws_ceil_div(h_sizes[t], SGD_CHUNK) : 0;
    return slots;
}

int ws_grad_norm(const float* const* h_grads, const int64_t* h_sizes, int32_t count, float max_norm, float* slots, int64_t nslots,
                 float* out, void* stream)
{
    WS_REQUIRE(count >= 0 && (count == 0 || (h_grads && h_sizes)), "bad tensor count %d or NULL argument", count);
    WS_REQUIRE(out, "NULL output");
    WS_REQUIRE(max_norm > 0.0f, "max_norm must be positive (got %g)", (double)max_norm);
    const int64_t need = ws_grad_norm_slots(h_sizes, count);
    WS_REQUIRE(need < (1ll << 31), "too many slots (%lld)", (long long)need);
    WS_REQUIRE(nslots >= need && (need == 0 || slots), "%lld slots given, %lld needed", (long long)nslots, (long long)need);
    hipStream_t st = (hipStream_t)stream;
    int t = 0, slot0 = 0;
    while (t < count) {
        NormArgs a;
        int blocks;
        if (int rc = fill_table(a, h_sizes, count, t, blocks, [&](int j, int src) {
                WS_REQUIRE(h_grads[src], "NULL tensor %d", src);
                a.g[j] = h_grads[src];
                return (int)WS_OK;
            })) return rc;
        if (a.count == 0) break;
        grad_sumsq_kernel<<<blocks, 256, 0, st>>>(a, slots, slot0);
        WS_LAUNCH_CHECK();
        slot0 += blocks;
    }
    grad_norm_finish_kernel<<<1, 64, 0, st>>>(slots, (int)need, max_norm, out);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_sgd_step_scaled(float* const* h_params, float* const* h_grads, float* const* h_bufs, const int64_t* h_sizes, int32_t count,
                       float lr, float momentum, float weight_decay, const float* coef, int32_t first, void* stream)
{
    WS_REQUIRE(count >= 0, "bad tensor count %d", count);
    if (count == 0) return WS_OK;
    WS_REQUIRE(h_params && h_grads && h_sizes && coef, "NULL argument");
    WS_REQUIRE(momentum == 0.0f || h_bufs, "momentum needs the momentum buffers");
    hipStream_t st = (hipStream_t)stream;
    int t = 0;
    while (t < count) {
        SgdArgs a;
        int blocks;
        if (int rc = fill_table(a, h_sizes, count, t, blocks, [&](int j, int src) {
                WS_REQUIRE(h_params[src] && h_grads[src] && (momentum == 0.0f || h_bufs[src]), "NULL tensor %d", src);
                a.p[j] = h_params[src];
                a.g[j] = h_grads[src];
                a.buf[j] = momentum != 0.0f ? h_bufs[src] : nullptr;
                return (int)WS_OK;
            })) return rc;
        if (a.count == 0) break;
        sgd_step_kernel<true><<<blocks, 256, 0, st>>>(a, lr, momentum, weight_decay, 0.0f, first, coef);
        WS_LAUNCH_CHECK();
    }
    return WS_OK;
}

int ws_sgd_step(float* const* h_params, const float* const* h_grads, float* const* h_bufs, const int64_t* h_sizes, int32_t count,
                float lr, float momentum, float weight_decay, float clip_value, int32_t first, void* stream)
{
    WS_REQUIRE(count >= 0, "bad tensor count %d", count);
    if (count == 0) return WS_OK;
    WS_REQUIRE(h_params && h_grads && h_sizes, "NULL argument");
    WS_REQUIRE(momentum == 0.0f || h_bufs, "momentum needs the momentum buffers");
    hipStream_t st = (hipStream_t)stream;
    int t = 0;
    while (t < count) {
        SgdArgs a;
        a.count = 0;
        int blocks = 0;
        while (t < count && a.count < SGD_MAX) {
            const int64_t n = h_sizes[t];
            WS_REQUIRE(n >= 0 && n < (1ll << 31) - SGD_CHUNK, "tensor %d too large (%lld elements)", t, (long long)n);
            if (n > 0) {
                WS_REQUIRE(h_params[t] && h_grads[t] && (momentum == 0.0f || h_bufs[t]), "NULL tensor %d", t);
                const int j = a.count++;
                a.p[j] = h_params[t];
                a.g[j] = h_grads[t];
                a.buf[j] = momentum != 0.0f ? h_bufs[t] : nullptr;
                a.n[j] = (int)n;
                a.first_block[j] = blocks;
                blocks += (int)ws_ceil_div(n, SGD_CHUNK);
            }
            ++t;
        }
        if (a.count == 0) break;
        a.first_block[a.count] = blocks;
        sgd_step_kernel<false><<<blocks, 256, 0, st>>>(a, lr, momentum, weight_decay, clip_value, first, nullptr);
        WS_LAUNCH_CHECK();
    }
    return WS_OK;
}

}  // extern "C"
