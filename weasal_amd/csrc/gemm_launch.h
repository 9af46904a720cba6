// weasal_amd/csrc/gemm_launch.h -- what crosses from gemm.hip (entries, checks, plans) into the dense-product family units: the
// plan records, the constants a plan and a kernel both read, and one launch_* function per kernel launch.  A kernel is
// instantiated where its dispatch(...) is, so each launch_* function -- its Pick<> / Flag lists and its if constexpr filter are
// the set of instantiations -- is defined in the unit that holds the kernel.  Nothing here is device code: the kernel argument
// types (XbGate, the group records) are gemm_device.h's and the family units', which gemm.hip does not include -- a launch_*
// function takes the problem record and builds them itself.
#pragma once
#include "ws_dispatch.h"

namespace gemm {

constexpr int BM = 128;   // rows of X per workgroup (32 per wave)
constexpr int BK = 32;    // k depth per LDS tile
constexpr int GROUP_MAX = 8;    // problems behind one grouped launch (GroupIndex, gemm_device.h)

// row stride of the small matrix (b_row_stride < 0: row-major [K, N])
inline int64_t xb_brs(const ws_xb_problem& q) { return q.b_row_stride < 0 ? q.n : q.b_row_stride; }

// The launch a product takes: every selection rule of the xb entries, shared with the reporter ws_gemm_xb_variant (which
// only reads the pointers' alignment).
enum { XB_NONE = 0, XB_XB2 = 1, XB_SHALLOW = 2, XB_GENERIC = 3 };
struct XbPlan {
    int kind;
    int nt, wn;             // XB_XB2: gemm_xb2_kernel<nt, wn>; XB_GENERIC: gemm_xb_kernel<nt, 32>
    dim3 grid;
    int splits, csplit;     // XB_XB2: split-K layers (splits > 1: sums in scratch, then splitk_epilogue_kernel), chunks per layer
    int staged;             // XB_XB2: ws_gemm_staged
    int vecx, vecb;         // XB_GENERIC: float4 loads of x / b
    int rows;               // XB_SHALLOW: rows per workgroup
    size_t lds;             // XB_SHALLOW: dynamic LDS bytes
};

// the (NT, WN) of gemm_xb2_kernel / gemm_xb2_group_kernel that exist; the index is the bucket of the grouped entry
constexpr int XB2_PAIRS[][2] = {{1, 1}, {2, 1}, {4, 1}, {1, 2}, {2, 2}};
constexpr int XB2_NPAIRS = 5;
constexpr int xb2_pair(int nt, int wn)
{
    for (int i = 0; i < XB2_NPAIRS; ++i)
        if (XB2_PAIRS[i][0] == nt && XB2_PAIRS[i][1] == wn) return i;
    return -1;
}
inline int xb2_no_instantiation(const XbPlan& p) { return ws_no_instantiation("gemm_xb2_kernel<NT=%d, WN=%d>", p.nt, p.wn); }

// The launches of a dW reduction: every selection rule of the xty entries, shared with the reporter ws_gemm_xty_variant
// (which only reads the pointers' alignment).  bf16: 2-byte operands (no gemm_xty_kernel fallback).
struct XtyPlan {
    int bf16;
    int lds;                // 0: gemm_xty2_kernel<kt, nt, wk, wn>; 1: gemm_xty_kernel<nt, kt> (32-bit buffer offsets overflow)
    int kt, nt, wk, wn;
    int vecx, vecy;         // gemm_xty_kernel: float4 loads
    int64_t chunk;
    int chunks;
    float* partial;         // out itself (one chunk, flat) or the scratch
    int reduce;             // 0: none, 1: reduce_partials_kernel, 2: reduce_partials_wide_kernel
    bool pitched;           // ldo > n: `out` is a column block of a wider matrix (row pitch ldo): the chunk sums go through the scratch
    dim3 grid;              //   and the reduction writes the pitched rows (also for one chunk, where it is the copy a caller would make)
};

// The launches of act_bwd_colsum_impl (m > 0), shared with the reporter ws_act_bwd_colsum_variant
struct ColsumPlan {
    int v;                  // act_bwd_colsum_kernel<v>: 4 = float4 columns, 1 = any n
    int64_t chunk;
    int chunks;
    float* partial;         // NULL (no column sums), colsum itself (one chunk) or the scratch
    int reduce;             // 1: reduce_partials_kernel adds the chunks
    dim3 grid;
};

// ---- the launches of a plan on `st`: the entry has validated and planned.  A function that makes ONE launch checks and counts
//      nothing -- the entry ends with WS_LAUNCH_CHECK; the grouped ones pass their own checks (one counted launch per group
//      launch: gemm_xb.hip).  WS_OK, or ws_no_instantiation's error.  Internal to the library (hidden: not part of its exports).
#pragma GCC visibility push(hidden)
// gemm_xb.hip (p.kind says which; launch_splitk_epilogue: the epilogue of ONE split product, p.splits > 1)
int launch_xb2(const ws_xb_problem& q, const XbPlan& p, hipStream_t st);
void launch_splitk_epilogue(const ws_xb_problem& q, const XbPlan& p, hipStream_t st);
void launch_xb_shallow(const ws_xb_problem& q, const XbPlan& p, hipStream_t st);
int launch_xb_generic(const ws_xb_problem& q, const XbPlan& p, hipStream_t st);
int launch_xb2_group(const ws_xb_problem* q, const XbPlan* plan, const int* ids, int cnt, hipStream_t st);
// gemm_xty.hip (launch_reduce_partials: wide = reduce_partials_wide_kernel, the plan's reduce == 2; n = ldo = 0: a flat output)
int launch_xty2(const ws_xty_problem& q, const XtyPlan& p, hipStream_t st);
int launch_xty_lds(const ws_xty_problem& q, const XtyPlan& p, hipStream_t st);
void launch_reduce_partials(bool wide, const float* partial, int64_t elems, int chunks, float* out, hipStream_t st, int n = 0,
                            int64_t ldo = 0);
int launch_xty2_group(const ws_xty_problem* q, const XtyPlan* plan, const int* ids, int cnt, hipStream_t st);
void launch_reduce_group(const ws_xty_problem* q, const XtyPlan* plan, const int* ids, int cnt, hipStream_t st);
// gemm_colsum.hip
int launch_act_bwd_colsum(const ColsumPlan& p, const float* dy, int64_t m, int32_t n, int64_t lddy, const float* y, int64_t ldy,
                          float slope, float* dz, int64_t lddz, const WsDrop& drop, hipStream_t st);
#pragma GCC visibility pop

}  // namespace gemm
