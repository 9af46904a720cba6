// weasal_amd/csrc/ws_scan.h -- device-wide exclusive prefix sum (int32) used by the table builders.
// Three-level reduce-then-scan: 4096 items per 256-thread workgroup, block sums scanned
// recursively.  scratch must hold ws_scan_scratch_items(n) int32.
#pragma once
#include "ws_common.h"

constexpr int WS_SCAN_BLOCK = 256;
constexpr int WS_SCAN_IPT = 16;
constexpr int WS_SCAN_TILE = WS_SCAN_BLOCK * WS_SCAN_IPT;

inline int64_t ws_scan_scratch_items(int64_t n)
{
    int64_t total = 2;
    while (n + 1 > WS_SCAN_TILE) {
        const int64_t t = ws_ceil_div(n + 1, WS_SCAN_TILE);
        total += t + 1;
        n = t;
    }
    return total;
}

// out[i] = sum_{j<i} in[i]; out has n+1 entries (out[n] = total).  in may alias out.
int ws_exclusive_scan_i32(const int32_t* in, int32_t* out, int64_t n, int32_t* scratch, hipStream_t st);

#ifdef __HIPCC__
// exclusive prefix of one int per thread inside a WS_SCAN_BLOCK-thread workgroup (scan.hip, sampler.hip)
__device__ __forceinline__ int ws_block_exclusive_scan(int v, int* lds /*[WS_SCAN_BLOCK/64 + 1]*/, int& block_total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    int wave_off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < WS_SCAN_BLOCK / 64; ++w) {
        const int s = lds[w];
        if (w < wave) wave_off += s;
        total += s;
    }
    __syncthreads();
    block_total = total;
    return wave_off + inc - v;
}
#endif
