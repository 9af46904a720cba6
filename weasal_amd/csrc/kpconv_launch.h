// weasal_amd/csrc/kpconv_launch.h -- what crosses from kpconv.hip (entries, checks, plans) into the kernel family units: the
// plan, the view of the search grid, and one launch_* function per kernel template.  A kernel is instantiated where its
// dispatch(...) is, so each launch_* function -- its Pick<> / Flag lists and its if constexpr filter are the set of
// instantiations -- is defined in the unit that holds the kernel.
#pragma once
#include "kpconv_device.h"

namespace kpconv {

// what a launcher launches; filled by the plan functions of kpconv.hip, read by launch_* and plan_text
enum { GK_FWD_MFMA, GK_FWD_POOL, GK_BWD_X, GK_BWD_GEOM, GK_BWD_X_GRID, GK_BWD_X_GRIDW, GK_BWD_GEOM_DEF, GK_BWD_X_PACKED };
#define WS_KP_SIZES 9, 13, 15     // the kernel sizes K the gather families instantiate
struct GatherPlan {
    int kernel;         // GK_*: the kernel family
    bool bf16;          // row type T: bf16_t instead of float
    int k;              // K: kernel points (WS_KP_SIZES; f32 rows and MODE 0 / 1 for the sizes other than 15)
    int n;              // NT (GK_FWD_MFMA), CK (GK_BWD_GEOM_DEF), G (the others; GK_BWD_GEOM has none)
    int mode;           // MODE
    bool def;           // DEF (the forward kernels)
    bool vec;           // VEC: float4 / 4 x bf16 row pieces (GK_FWD_MFMA: VECROW, always true; GK_BWD_GEOM: the argument vec4)
    int pw;             // PW (GK_FWD_POOL)
    bool cut;           // CUT (GK_FWD_MFMA, GK_BWD_GEOM_DEF)
    int nch;            // NCH (GK_BWD_X_GRIDW)
    bool sort;          // SORT (GK_BWD_X_GRID)
    bool areg;          // AREG (GK_BWD_GEOM_DEF)
    int grid;           // workgroups of 256 threads
    int csplit, ilv, rows_sorted;   // GeomParams::csplit (1 = a query is one item), ::ilv, ::cut
};

// the grid blob of the search (ws_grid.h) as K4G reads it
struct GridView {
    const CloudGrid* grids;
    const int32_t* cell_start;
    const float4* sorted;
    const unsigned long long* key_last;
    float r2;
};
inline GridView grid_view(const void* grid_blob, int32_t nb, int64_t cells, const uint64_t* key_last, float radius)
{
    const char* base = (const char*)grid_blob;
    return GridView{(const CloudGrid*)base, (const int32_t*)(base + ws_grid_blob_cells_off(nb)),
                    (const float4*)(base + ws_grid_blob_sorted_off(nb, cells)), reinterpret_cast<const unsigned long long*>(key_last),
                    radius * radius};                       // neighbors.cpp:226, as in the search
}

// ---- one kernel launch each on `stream`, nothing checked and nothing counted: the entry has validated and planned, and ends
//      with WS_LAUNCH_CHECK.  Internal to the library (hidden: not part of its exports).
#pragma GCC visibility push(hidden)
// kpconv_fwd.hip
void launch_fwd_mfma(const GatherPlan& p, void* stream, const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int64_t* inds,
                     int32_t h, const void* x, int32_t ci, const float* kernel_points, const float* deformed_kp, const float* modulations,
                     const GeomParams& g, void* wf, float* min_d2, const int32_t* order);
void launch_fwd_pool(const GatherPlan& p, void* stream, const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int64_t* inds,
                     int32_t h, const void* x, int32_t ci, const float* kernel_points, const float* deformed_kp, const float* modulations,
                     const GeomParams& g, void* wf, float* min_d2, const int32_t* order);
void launch_fwd_fused(void* stream, const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int64_t* inds, int32_t h,
                      const float* x, int32_t ci, const float* kernel_points, const GeomParams& g, const int32_t* order, const FuseArgs& fz);
// kpconv_bwd_x.hip
void launch_bwd_x(const GatherPlan& p, void* stream, const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, int32_t h,
                  const int32_t* t_offsets, const int32_t* t_pairs, const void* dwf, int32_t ci, const float* kernel_points,
                  const float* deformed_kp, const float* modulations, const GeomParams& g, void* dx, const int32_t* order);
void launch_bwd_x_packed(const GatherPlan& p, void* stream, const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, int32_t h,
                         const int32_t* t_offsets, const int32_t* t_pairs, const float* dwf, int32_t ci, const float* kernel_points,
                         const GeomParams& g, float* dx, const int32_t* order);
// kpconv_bwd_geom.hip
void launch_bwd_geom(const GatherPlan& p, void* stream, const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int64_t* inds,
                     int32_t h, const void* x, int32_t ci, const void* dwf, const float* deformed_kp, const float* modulations,
                     const float* d_min_d2, const GeomParams& g, float* d_deformed_kp, float* d_modulations);
void launch_bwd_geom_def(const GatherPlan& p, void* stream, const float* q_pts, int64_t nq, const float* s_pts, int64_t ns,
                         const int64_t* inds, int32_t h, const void* x, int32_t ci, const void* dwf, const float* kp4, const float* d_min_d2,
                         float extent, float* d_kp4, const int32_t* order);
// kpconv_bwd_grid.hip; launch_bwd_x_grid_k<KN>: kpconv_bwd_grid_kernels.h, one unit per kernel size
template <int KN>
void launch_bwd_x_grid_k(const GatherPlan& p, void* stream, const float* s_pts, int64_t ns, const GridView& v, int32_t nb, const void* dwf,
                         int32_t ci, const float* kernel_points, const float* deformed_kp, const float* modulations, const GeomParams& g,
                         void* dx, const int32_t* order, int32_t* overflow);
void launch_bwd_x_grid(const GatherPlan& p, void* stream, const float* s_pts, int64_t ns, const GridView& v, int32_t nb, const void* dwf,
                       int32_t ci, const float* kernel_points, const float* deformed_kp, const float* modulations, const GeomParams& g,
                       void* dx, const int32_t* order, int32_t* overflow);
// kpconv_bwd_gridw.hip
void launch_bwd_x_gridw(const GatherPlan& p, void* stream, const float* s_pts, int64_t ns, const GridView& v, int32_t nb, const void* dwf,
                        int32_t ci, const float* kernel_points, const GeomParams& g, void* dx, const int32_t* order);
void launch_kp4_rmax(void* stream, const float* kp4, int64_t n, float* rmax);      // the helper of the wide-grid entry; rmax zeroed before
#pragma GCC visibility pop

}  // namespace kpconv
