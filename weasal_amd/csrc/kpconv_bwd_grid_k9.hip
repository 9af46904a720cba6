// weasal_amd/csrc/kpconv_bwd_grid_k9.hip -- K4G, the slab form (kpconv_bwd_grid_kernels.h): the unit of K = 9 (f32 rows)
#include "kpconv_bwd_grid_kernels.h"

namespace kpconv {
WS_BWD_X_GRID_UNIT(9)
}  // namespace kpconv
