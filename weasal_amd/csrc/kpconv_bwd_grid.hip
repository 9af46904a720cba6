// weasal_amd/csrc/kpconv_bwd_grid.hip -- K4G, the slab form (kpconv_bwd_grid_kernels.h): the unit of K = 15, and the launcher of
// the entries, which hands a plan to the unit of its kernel size.
#include "kpconv_bwd_grid_kernels.h"

namespace kpconv {

WS_BWD_X_GRID_UNIT(15)
extern template void launch_bwd_x_grid_k<9>(const GatherPlan&, void*, const float*, int64_t, const GridView&, int32_t, const void*, int32_t,
                                            const float*, const float*, const float*, const GeomParams&, void*, const int32_t*, int32_t*);
extern template void launch_bwd_x_grid_k<13>(const GatherPlan&, void*, const float*, int64_t, const GridView&, int32_t, const void*, int32_t,
                                             const float*, const float*, const float*, const GeomParams&, void*, const int32_t*, int32_t*);

void launch_bwd_x_grid(const GatherPlan& p, void* stream, const float* s_pts, int64_t ns, const GridView& v, int32_t nb, const void* dwf,
                       int32_t ci, const float* kernel_points, const float* deformed_kp, const float* modulations, const GeomParams& g,
                       void* dx, const int32_t* order, int32_t* overflow)
{
    dispatch([&](auto kn) {
        launch_bwd_x_grid_k<kn.value>(p, stream, s_pts, ns, v, nb, dwf, ci, kernel_points, deformed_kp, modulations, g, dx, order, overflow);
    }, Pick<WS_KP_SIZES>{p.k});
}

}  // namespace kpconv
