// weasal_amd/csrc/nearest_kernels.h -- exact nearest support of every query, no radius (ws_nearest_neighbors): the device side.
// Included by neighbors.hip alone, behind neighbors_kernels.h (the workspace's counting-sort grid is the one K1 builds).
//
// Replaces sklearn's KDTree.query(points, k=1) (datasets/DALES_PseudoLabel.py:888-893).  The key a query minimises is
// (d2, j): d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in float64 with dx = (double)q.x - (double)s.x, every product and sum rounded
// (no FMA), ties to the smallest global index.  The minimum of a key over a set does not depend on the order of the visit,
// so which cells a query walks decides only WHEN it may stop, never what it returns.
//
// Work assignment: one LANE per query.  With a cell that holds a few supports the 27 cells around a query hold a dozen
// candidates: a wave (nb_nearest_kernel) or a quarter-wave per query would leave most lanes masked, and a lane-per-query
// walk needs no cross-lane step at all -- the result path has no shuffle, no LDS and no atomic.  The loads are 16-byte
// gathers from the cell-sorted copy; neighbouring queries (file order of a tile, or the cell order of a self-query)
// share their cells through L2.  The price is divergence: a wave waits for its longest walk.
#pragma once
#include "neighbors_kernels.h"

namespace {

// Cell size of the exact search when the caller passes cell = 0: per element the smallest cell of the
// series (largest extent / 512) * 1.26^k whose grid has at most max(1, 2 s_len) cells (and, as every grid, at most 512
// cells per axis and cell_cap cells): about half a support per cell of the box, a few per occupied cell of a surface-like
// cloud.  Only the speed depends on it.
__global__ void nn_grid_setup_kernel(CloudGrid* __restrict__ grids, const float* __restrict__ bbox, int nb)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    CloudGrid g = grids[b];
    if (g.s_len <= 0) {
        g.lo[0] = g.lo[1] = g.lo[2] = 0.f; g.inv_cell = 1.f; g.nx = g.ny = g.nz = 1;
        grids[b] = g;
        return;
    }
    const float* bb = bbox + 6 * b;
    const float ext = fmaxf(fmaxf(bb[3] - bb[0], bb[4] - bb[1]), bb[5] - bb[2]);
    const int64_t want = min((int64_t)g.cell_cap, max((int64_t)1, 2 * (int64_t)g.s_len));
    float cell = ext > 0.f && ext < 3.0e38f ? ext * (1.001f / 512.0f) : 1.f;
    if (!(cell >= 1.0e-30f)) cell = 1.0e-30f;              // 1 / cell stays finite
    int nx = 1, ny = 1, nz = 1;
    bool ok = false;
    for (int it = 0; it < 1024 && !ok; ++it) {             // (a bounding box that is not finite never fits: one cell then)
        const float inv = 1.0f / cell;
        const float fx = floorf((bb[3] - bb[0]) * inv), fy = floorf((bb[4] - bb[1]) * inv), fz = floorf((bb[5] - bb[2]) * inv);
        ok = fx >= 0.f && fx < 512.f && fy >= 0.f && fy < 512.f && fz >= 0.f && fz < 512.f;
        if (ok) {
            nx = (int)fx + 1; ny = (int)fy + 1; nz = (int)fz + 1;
            ok = (int64_t)nx * ny * nz <= want;
        }
        if (!ok) cell *= 1.26f;
    }
    if (!ok) { nx = ny = nz = 1; cell = 1.f; }
    g.lo[0] = bb[0]; g.lo[1] = bb[1]; g.lo[2] = bb[2];
    g.inv_cell = 1.0f / cell;
    g.nx = nx; g.ny = ny; g.nz = nz;
    grids[b] = g;
}

// ns == 0 with nq > 0: every query answers "no support"
template <typename OutT>
__global__ __launch_bounds__(256) void nn_none_kernel(int64_t nq, int64_t ns, OutT* __restrict__ out, double* __restrict__ out_d2)
{
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
        out[q] = (OutT)ns;
        if (out_d2) out_d2[q] = __builtin_huge_val();
    }
}

// best key of one query so far
struct NnBest { double d2; int idx; };

// the candidates [beg, end) of the cell-sorted copy against the query
__device__ __forceinline__ NnBest nn_scan(NnBest best, int beg, int end, const float4* __restrict__ sorted, double qx, double qy, double qz)
{
#pragma clang fp contract(off)
    for (int p = beg; p < end; ++p) {
        const float4 c = sorted[p];
        const double dx = qx - (double)c.x, dy = qy - (double)c.y, dz = qz - (double)c.z;
        const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
        const double d2 = (xx + yy) + zz;
        const int j = __float_as_int(c.w);
        // a non-finite support gives inf or NaN and is never chosen; best.idx < 0: nothing chosen yet
        const bool better = d2 < __builtin_huge_val() && (d2 < best.d2 || (d2 == best.d2 && (best.idx < 0 || j < best.idx)));
        if (better) { best.d2 = d2; best.idx = j; }
    }
    return best;
}

// Stop rule.  The cells [c - k, c + k] (clipped to the grid) around the cell c have been visited.  A support that has not
// been seen lies in a cell beyond one of the six faces of that box, and only beyond a face that is not a face of the grid.
// Its computed cell coordinate t = fl(fl(s - lo) * inv_cell) is off the real one by at most 2^-23 * 512 < 1e-4 cells, so it
// lies farther from the query than the TRUE distance (float64, from lo and 1 / inv_cell) of the query to that face minus
// 1e-4 cells.  The bound is shrunk by 1e-3 cells (the 1.001 of nb_grid_setup_kernel: it dominates the rounding of
// cell_coord) and by 2^-40 relative (it dominates the float64 rounding of the bound and of d2 at any magnitude): when
// best <= bound^2, every unseen support has a strictly larger float64 d2.  +inf bound: the box covers the grid.
__device__ __forceinline__ bool nn_done(double best_d2, int k, int cx, int cy, int cz, const CloudGrid g, double cell,
                                        double ox, double oy, double oz)
{
#pragma clang fp contract(off)
    double bound = __builtin_huge_val();
    if (cx - k > 0) bound = fmin(bound, ox - (double)(cx - k) * cell);
    if (cx + k < g.nx - 1) bound = fmin(bound, (double)(cx + k + 1) * cell - ox);
    if (cy - k > 0) bound = fmin(bound, oy - (double)(cy - k) * cell);
    if (cy + k < g.ny - 1) bound = fmin(bound, (double)(cy + k + 1) * cell - oy);
    if (cz - k > 0) bound = fmin(bound, oz - (double)(cz - k) * cell);
    if (cz + k < g.nz - 1) bound = fmin(bound, (double)(cz + k + 1) * cell - oz);
    if (bound == __builtin_huge_val()) return true;
    bound = (bound - 1.0e-3 * cell) * (1.0 - 0x1p-40);
    return bound > 0.0 && best_d2 <= bound * bound;
}

// Skip rule, the same argument for one run of cells [a0, a1] along each axis: per axis the gap between the query and the
// cells' slab (0 inside it), shrunk as above; the sum of their squares is below the float64 d2 of every support of those
// cells.  A run whose bound is positive and not below the best d2 holds nothing that could win, not even a tie.
__device__ __forceinline__ double nn_gap(double o, int a0, int a1, double cell)
{
#pragma clang fp contract(off)
    const double gap = fmax(fmax((double)a0 * cell - o, o - (double)(a1 + 1) * cell), 0.0);
    return fmax(gap - 1.0e-3 * cell, 0.0) * (1.0 - 0x1p-40);
}
__device__ __forceinline__ bool nn_skip(double best_d2, double gx, double gy, double gz)
{
#pragma clang fp contract(off)
    const double bound2 = ((gx * gx) + (gy * gy)) + (gz * gz);
    return bound2 > 0.0 && best_d2 <= bound2;
}

// One lane per query.  The 3x3x3 block comes through grid_cell_runs (the rule of which cells a point sees, ws_grid.h); it
// is the box of Chebyshev radius 1 exactly when the query's own cell coordinates are inside the grid: then the centre row
// goes first and the other eight are held against the skip rule.  A query outside (cell_coord clamps at -2 and 1e6: the raw
// coordinate says nothing about the distance) keeps whatever that block held and starts its shells at radius 0 around the
// CLAMPED cell; the bounds come from the true geometry either way.  Shell k is the box of radius k without the box of
// radius k - 1, as runs of cells contiguous in x, each held against the skip rule.  At most max(nx, ny, nz) shells,
// whatever the coordinates: after them the box covers the grid.  status: bit WS_NN_STATUS_NONFINITE_QUERY.
template <typename OutT>
__global__ __launch_bounds__(256) void nn_exact_kernel(const float* __restrict__ queries, int64_t nq,
                                                        const CloudGrid* __restrict__ grids, int nb,
                                                        const int32_t* __restrict__ cell_start,
                                                        const float4* __restrict__ sorted, int64_t ns,
                                                        const int32_t* __restrict__ qorder, OutT* __restrict__ out,
                                                        double* __restrict__ out_d2, int32_t* __restrict__ status)
{
#pragma clang fp contract(off)
    int b = 0;
    CloudGrid g = grids[0];
    bool bad = false;
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < nq; it += (int64_t)gridDim.x * 256) {
        const int64_t q = qorder ? (int64_t)qorder[it] : it;
        if (q < g.q_base || q >= g.q_base + g.q_len) {
            b = find_cloud_q(grids, nb, q);
            g = grids[b];
        }
        const float qx = queries[3 * q], qy = queries[3 * q + 1], qz = queries[3 * q + 2];
        NnBest best{__builtin_huge_val(), -1};
        const bool finite = fabsf(qx) < __builtin_huge_valf() && fabsf(qy) < __builtin_huge_valf() && fabsf(qz) < __builtin_huge_valf();
        if (!finite) {
            bad = true;
        } else if (g.s_len > 0) {
            const double dqx = (double)qx, dqy = (double)qy, dqz = (double)qz;
            const CellRuns u = grid_cell_runs(g, qx, qy, qz, cell_start);
            const int rx = cell_coord(qx, g.lo[0], g.inv_cell);
            const int ry = cell_coord(qy, g.lo[1], g.inv_cell);
            const int rz = cell_coord(qz, g.lo[2], g.inv_cell);
            const int cx = min(max(rx, 0), g.nx - 1), cy = min(max(ry, 0), g.ny - 1), cz = min(max(rz, 0), g.nz - 1);
            const bool inside = rx == cx && ry == cy && rz == cz;
            const double cell = 1.0 / (double)g.inv_cell;
            const double ox = dqx - (double)g.lo[0], oy = dqy - (double)g.lo[1], oz = dqz - (double)g.lo[2];
            best = nn_scan(best, u.rb[4], u.re[4], sorted, dqx, dqy, dqz);
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                if (r == 4) continue;
                // (the x range of a run holds the query's own cell: no gap along x; only an inside query knows its rows)
                if (inside && nn_skip(best.d2, 0.0, nn_gap(oy, cy + r % 3 - 1, cy + r % 3 - 1, cell),
                                      nn_gap(oz, cz + r / 3 - 1, cz + r / 3 - 1, cell)))
                    continue;
                best = nn_scan(best, u.rb[r], u.re[r], sorted, dqx, dqy, dqz);
            }
            const int kmax = max(g.nx, max(g.ny, g.nz));
            int k = inside ? 1 : -1;                                 // radius of the box visited so far
            for (;;) {
                if (k >= 0 && nn_done(best.d2, k, cx, cy, cz, g, cell, ox, oy, oz)) break;
                ++k;
                if (k >= kmax) break;                                // every cell has been seen
                const int xa = cx - k, xb = cx + k;
                const int xlo = max(xa, 0), xhi = min(xb, g.nx - 1);
                for (int z = max(cz - k, 0); z <= min(cz + k, g.nz - 1); ++z) {
                    const double gz = nn_gap(oz, z, z, cell);
                    for (int y = max(cy - k, 0); y <= min(cy + k, g.ny - 1); ++y) {
                        const double gy = nn_gap(oy, y, y, cell);
                        const int row = g.cell_base + (z * g.ny + y) * g.nx;
                        if (z - cz == k || cz - z == k || y - cy == k || cy - y == k) {      // a y or z face of the shell: the whole x run
                            if (!nn_skip(best.d2, nn_gap(ox, xlo, xhi, cell), gy, gz))
                                best = nn_scan(best, cell_start[row + xlo], cell_start[row + xhi + 1], sorted, dqx, dqy, dqz);
                        } else {                                                          // the two x faces
                            if (xa >= 0 && !nn_skip(best.d2, nn_gap(ox, xa, xa, cell), gy, gz))
                                best = nn_scan(best, cell_start[row + xa], cell_start[row + xa + 1], sorted, dqx, dqy, dqz);
                            if (xb < g.nx && !nn_skip(best.d2, nn_gap(ox, xb, xb, cell), gy, gz))
                                best = nn_scan(best, cell_start[row + xb], cell_start[row + xb + 1], sorted, dqx, dqy, dqz);
                        }
                    }
                }
            }
        }
        out[q] = best.idx >= 0 ? (OutT)best.idx : (OutT)ns;
        if (out_d2) out_d2[q] = best.d2;
    }
    if (status && bad) atomicOr(status, WS_NN_STATUS_NONFINITE_QUERY);
}

}  // namespace
