// weasal_amd/csrc/ws_grid.h -- the uniform cell grid of the radius search and the walk over it, shared by K1
// (neighbors_kernels.h) and the table-free KPConv backward (kpconv_bwd_grid_kernels.h, kpconv_bwd_gridw.hip):
//   cell_coord, ref_d2                      the floating-point steps that decide a cell or a distance;
//   grid_cell_block / _run / _runs          the 3x3x3 block around a point as nine cell runs, with the clamp that makes
//                                           the loads unconditional (the one place that says which cells a point sees);
//   grid_walk                               nine first batches in flight, then the tails, for a candidate functor;
//   nb_key, nb_key_index, nb_key_d2         the (distance, index) key of a row entry and of key_last;
//   lane_rank, slab_compact, wave_lds_sync  ballot compaction into a wave's LDS slab.
// Every floating-point step that decides a cell or a distance sits under `#pragma clang fp contract(off)`, so the
// translation units produce the same bits whatever their -ffp-contract setting (the reference's recipe has no FMA:
// nanoflann.hpp:432-440; HIP's __fmul_rn / __fadd_rn are plain operators and do NOT stop the contraction).
// The helpers take the grid and their other inputs BY VALUE and return values: a kernel that hands its CloudGrid to a
// helper by reference keeps it in memory through the early optimisation passes and comes out as different code
// (+ 50 .. 100 instructions in the fill kernels); tools/codegen_diff.py against the previous build is the check.
#pragma once
#include "ws_common.h"

struct CloudGrid {        // one per batch element, device resident
    float lo[3];
    float inv_cell;
    int nx, ny, nz;
    int cell_base;        // first cell of this element in the global cell arrays
    int cell_cap;         // cells reserved for this element
    int s_base, s_len;
    int q_base, q_len;
};

#ifdef __HIPCC__
// cell coordinate; clamped so that far-away queries cannot overflow the int conversion
__device__ __forceinline__ int cell_coord(float v, float lo, float inv)
{
#pragma clang fp contract(off)
    const float d = v - lo;
    const float t = floorf(d * inv);
    return (int)fminf(fmaxf(t, -2.0f), 1.0e6f);
}

// exact reference recipe (nanoflann.hpp:432-440): result = 0; result += diff*diff, diff = query - support
__device__ __forceinline__ float ref_d2(float qx, float qy, float qz, const float4& c)
{
#pragma clang fp contract(off)
    const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    float r = xx;
    r = r + yy;
    r = r + zz;
    return r;
}

// The (distance, index) key K1 sorts a row by and the grid-walk backward compares with key_last: d2 >= 0, so its IEEE
// bit pattern is monotonic; ties fall back to the index.  The only place that knows the layout.
__device__ __forceinline__ unsigned long long nb_key(float d2, unsigned idx)
{
    return ((unsigned long long)__float_as_uint(d2) << 32) | idx;
}
__device__ __forceinline__ unsigned nb_key_index(unsigned long long key) { return (unsigned)(key & 0xffffffffull); }
__device__ __forceinline__ float nb_key_d2(unsigned long long key) { return __uint_as_float((unsigned)(key >> 32)); }

// a slab private to one wave: order the wave's own LDS writes before its reads
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// number of set bits of the ballot `m` below this lane: the lane's place among the hits of its batch
__device__ __forceinline__ int lane_rank(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// Compaction step of a candidate batch: the hits go to slab[cnt ...] in lane order, misses and hits beyond `cap` to the
// lane's dummy slot slab[cap + lane] (branch free: exec-mask branches cost the scalar unit more than the store costs
// the LDS).  Every lane of the wave takes part.  Returns (the lane's slot, cnt advanced by the number of hits); the
// caller stores its value at the slot.
__device__ __forceinline__ int2 slab_compact(bool hit, int cap, int lane, int cnt)
{
    const unsigned long long m = __ballot(hit);
    const int pos = cnt + lane_rank(m);
    const int slot = (hit && pos < cap) ? pos : cap + lane;
    return make_int2(slot, cnt + __builtin_popcountll(m));
}

// The 3x3x3 cell block around a point is nine runs of cells contiguous in x: the x range and the centre row.
struct CellBlock { int x0, x1, cy, cz; };
__device__ __forceinline__ CellBlock grid_cell_block(const CloudGrid g, float x, float y, float z)
{
    const int cx = cell_coord(x, g.lo[0], g.inv_cell);
    const int cy = cell_coord(y, g.lo[1], g.inv_cell);
    const int cz = cell_coord(z, g.lo[2], g.inv_cell);
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.nx - 1);
    return CellBlock{x0, x1, cy, cz};
}
// Run r (0 .. 8) of the block as [begin, end) in the cell-sorted copy.  A run outside the grid is empty (0, 0) and its
// row is clamped to row 0, which is what makes the loads unconditional and safe.  THE rule of which cells a point sees:
// K1 and the grid-walk backward must walk the same cells, or dx silently loses pairs.
__device__ __forceinline__ int2 grid_cell_run(const CloudGrid g, const CellBlock k, int r, const int32_t* __restrict__ cell_start)
{
    const int z = k.cz + r / 3 - 1, y = k.cy + r % 3 - 1;
    const bool ok = k.x0 <= k.x1 && z >= 0 && z < g.nz && y >= 0 && y < g.ny;
    const int row = g.cell_base + ((ok ? z : 0) * g.ny + (ok ? y : 0)) * g.nx;
    const int rb = ok ? cell_start[row + k.x0] : 0;
    const int re = ok ? cell_start[row + k.x1 + 1] : 0;
    return make_int2(rb, re);
}
struct CellRuns { int rb[9], re[9]; };
__device__ __forceinline__ CellRuns grid_cell_runs(const CloudGrid g, float x, float y, float z, const int32_t* __restrict__ cell_start)
{
    const CellBlock k = grid_cell_block(g, x, y, z);
    CellRuns u;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const int2 run = grid_cell_run(g, k, r, cell_start);
        u.rb[r] = run.x;
        u.re[r] = run.y;
    }
    return u;
}

// Walk the candidates of the point (x, y, z): f(float4 cand, bool active) for all lanes in lock-step, `cand.w` carries
// the global support index.  The first 64 candidates of the nine runs are fetched together (nine independent gathers in
// flight instead of nine dependent round trips), then the tails of runs longer than one wave.  Needs g.s_len > 0: the
// masked lanes read entry 0.  nb_fill128_kernel walks through it; nb_nearest_kernel and kpconv_gather_bwd_x_grid_kernel
// spell the same two loops out over grid_cell_runs (through the functor their tail loops come out laid out differently).
template <typename F>
__device__ __forceinline__ void grid_walk(const CloudGrid g, float x, float y, float z, const int32_t* __restrict__ cell_start,
                                          const float4* __restrict__ sorted, int lane, F f)
{
    const CellRuns u = grid_cell_runs(g, x, y, z, cell_start);
    float4 c[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const int p = u.rb[r] + lane;
        c[r] = sorted[p < u.re[r] ? p : 0];          // unconditional, masked by `active`
    }
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        f(c[r], u.rb[r] + lane < u.re[r]);
        for (int p0 = u.rb[r] + 64; p0 < u.re[r]; p0 += 64) {      // runs longer than one wave (dense cells)
            const int p = p0 + lane;
            float4 cc = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p < u.re[r]) cc = sorted[p];
            f(cc, p < u.re[r]);
        }
    }
}

// layout of an exported grid (ws_radius_neighbors_grid_export): [CloudGrid nb | cell_start cells+2 | sorted ns]
__host__ __device__ inline int64_t ws_grid_blob_align(int64_t b) { return (b + 255) / 256 * 256; }
__host__ __device__ inline int64_t ws_grid_blob_cells_off(int nb) { return ws_grid_blob_align((int64_t)nb * (int64_t)sizeof(CloudGrid)); }
__host__ __device__ inline int64_t ws_grid_blob_sorted_off(int nb, int64_t cells)
{
    return ws_grid_blob_cells_off(nb) + ws_grid_blob_align((cells + 2) * (int64_t)sizeof(int32_t));
}
__host__ __device__ inline int64_t ws_grid_blob_bytes(int nb, int64_t cells, int64_t ns)
{
    return ws_grid_blob_sorted_off(nb, cells) + ns * (int64_t)sizeof(float4);
}
#endif
