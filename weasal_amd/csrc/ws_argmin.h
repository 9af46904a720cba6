// weasal_amd/csrc/ws_argmin.h -- (smallest value, smallest index among equal values) of float64 data inside one
// 256-thread workgroup: the reduction of the sampling potentials shared by tester.hip (ws_potentials_update) and
// sampler.hip (ws_sampler_batch).  Only comparisons: every caller gets the same pair whatever the launch shape.
#pragma once
#include "ws_common.h"

#ifdef __HIPCC__
// fold (v, i) into the running (best, bi); an index < 0 stands for "nothing yet"
__device__ __forceinline__ void ws_argmin_take(double& best, long long& bi, double v, long long i)
{
    if (i >= 0 && (v < best || (v == best && (bi < 0 || i < bi)))) { best = v; bi = i; }
}

// tree reduction over the 256 threads of the workgroup; the result is in sv[0] / si[0] after the call (all threads)
__device__ __forceinline__ void ws_argmin_block(double best, long long bi, double* sv /*[256]*/, long long* si /*[256]*/)
{
    sv[threadIdx.x] = best;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const double ov = sv[threadIdx.x + o];
            const long long oi = si[threadIdx.x + o];
            if (oi >= 0 && (ov < sv[threadIdx.x] || (ov == sv[threadIdx.x] && (si[threadIdx.x] < 0 || oi < si[threadIdx.x])))) {
                sv[threadIdx.x] = ov;
                si[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
}
#endif
