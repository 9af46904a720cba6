// weasal_amd/csrc/kpconv.hip -- the C entries of the fused KPConv gather: checks, launch plans, reporters.
//
// Reference semantics: models/blocks.py:238-374 (KPConv.forward) and its autograd.
//
// K3  ws_kpconv_gather_fwd*      kpconv_fwd.hip        K4G  ws_kpconv_gather_bwd_x_grid*  kpconv_bwd_grid.hip, kpconv_bwd_gridw.hip (_wide)
// K4  ws_kpconv_gather_bwd_x*    kpconv_bwd_x.hip      K6   ws_kpconv_gather_bwd_geom*    kpconv_bwd_geom.hip
// No kernel is launched from this file: an entry validates, plans, and calls the launch_* function of the family unit
// (kpconv_launch.h), then passes the one launch check that counts it.  Every selection rule is here.
#include "kpconv_launch.h"
#include <algorithm>
#include <cstdio>

extern "C" int ws_kpconv_grid_sorted;     // 1: ws_kpconv_gather_bwd_x_grid sums the incoming pairs in index order (the pair order of
int ws_kpconv_grid_sorted = 0;            //    the transposed table: bit-identical to ws_kpconv_gather_bwd_x); 0: in grid-walk order

namespace {

constexpr int SPLIT_ROWS = 4096;   // matrix-core K3 on fewer queries than this: one item per (query, channel block)
constexpr int PACK_MEAN_MAX = 12;  // packed K4 up to this many incoming pairs per support on average (nq * h <= this * ns)
constexpr int SPLIT_NT = 4;        // ... with at most this many channels per lane (blocks of 16 x this many channels)
constexpr int GRID_INTERLEAVE = 512;   // K4G and the wide-row K4G of config 5: workgroups per XCD of the interleaved assignment

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the kernel sizes of this build (WS_KP_SIZES): 15 in every form; 9 and 13 with f32 rows through the generic forms (MODE 0 / 1).
// bf16 rows, the deformable fast path (MODE 2: the _def entries, packed kernel points) and the fused forward layer are 15 only.
bool built_k(int k)
{
    for (int v : {WS_KP_SIZES}) if (k == v) return true;
    return false;
}
bool supported_k(int k, bool bf16, int mode) { return built_k(k) && (k == 15 || (!bf16 && mode != 2)); }
int check_k(int k, bool bf16, int mode)
{
    if (!built_k(k)) return ws_fail(WS_ERR_UNSUPPORTED, "num_kernel_points=%d: this build instantiates K=9, K=13 and K=15", k);
    if (!supported_k(k, bf16, mode))
        return ws_fail(WS_ERR_UNSUPPORTED, "num_kernel_points=%d with %s: this build instantiates K=9, K=13 and K=15, and %s for K=15 only", k,
                       mode == 2 ? "packed kernel points" : "bf16 rows", mode == 2 ? "the deformable fast path (MODE 2)" : "bf16 rows");
    return WS_OK;
}

int check_common(const void* q_pts, int64_t nq, const void* s_pts, int64_t ns, int32_t h, int32_t ci,
                 int32_t k, float extent, int32_t influence, int32_t aggregation)
{
    WS_REQUIRE(nq >= 0 && ns >= 0, "negative point count (nq=%lld ns=%lld)", (long long)nq, (long long)ns);
    WS_REQUIRE(h >= 1 && ci >= 1, "h=%d and ci=%d must be >= 1", h, ci);
    WS_REQUIRE(nq == 0 || q_pts, "q_pts is NULL");
    WS_REQUIRE(ns == 0 || s_pts, "s_pts is NULL");
    WS_REQUIRE(extent > 0.0f, "KP_extent must be > 0");
    WS_REQUIRE(influence >= 0 && influence <= 2, "unknown influence %d", influence);
    WS_REQUIRE(aggregation >= 0 && aggregation <= 1, "unknown aggregation %d", aggregation);
    WS_REQUIRE(ns < (1ll << 31) && nq * (int64_t)k < (1ll << 31), "index range exceeds int32");
    return check_k(k, false, 0);
}

// ---- plans (GatherPlan, kpconv_launch.h): what a launcher launches, from its arguments alone (pointers only for their alignment).
//      The entries below and the reporters (ws_kpconv_gather_variant, ws_kpconv_gather_fwd_variant) call the same plan function;
//      every selection rule is here.
// NT of the matrix-core K3: channels per lane, from the row width; one channel per lane (any ci, any alignment: lanes past ci
// are masked) unless the rows split into NT-channel pieces
int nt_for_rows(int ci, const void* a, const void* b)
{
    const int nt = ci <= 16 ? 1 : (ci <= 32 ? 2 : (ci <= 64 ? 4 : (ci <= 128 ? 8 : 16)));
    return (ci % nt == 0 && (nt == 1 || (aligned16(a) && aligned16(b)))) ? nt : 1;
}
// G of K4 / K4G: groups of 4 channels per support
int group_ladder(int ci) { return ci <= 4 ? 1 : (ci <= 8 ? 2 : (ci <= 16 ? 4 : (ci <= 32 ? 8 : 16))); }
// VEC: both row sets move as float4 / 4 x bf16 pieces
bool rows_vec4(bool bf16, int ci, const void* a, const void* b)
{
    return ci % 4 == 0 && (bf16 ? ws_row_aligned<bf16_t>(a) && ws_row_aligned<bf16_t>(b) : ws_row_aligned<float>(a) && ws_row_aligned<float>(b));
}
// ... and bf16 rows have no other form (VEC = false is not instantiated for them)
int rows_vec4_or_f32(bool bf16, int ci, const void* a, const void* b, bool& vec4)
{
    vec4 = rows_vec4(bf16, ci, a, b);
    WS_REQUIRE(!bf16 || vec4, "bf16 feature rows need ci %% 4 == 0 and 8-byte aligned rows (ci=%d)", ci);
    return WS_OK;
}
// MODE 0 of the generic entries: rigid, not modulated, linear influence, sum
bool rigid_fast(bool deformed, bool modulated, int influence, int aggregation)
{
    return !deformed && !modulated && influence == WS_INFLUENCE_LINEAR && aggregation == WS_AGGREGATION_SUM;
}
// K4G: with a point order the supports are dealt out interleaved, GRID_INTERLEAVE workgroups per XCD
void grid_walk_plan(int64_t ns, bool ordered, GatherPlan& p)
{
    p.ilv = ordered ? GRID_INTERLEAVE : 0;
    p.grid = p.ilv > 0 ? 8 * (int)std::max<int64_t>(1, std::min<int64_t>(p.ilv, ws_ceil_div(ns, 32))) : ws_grid(ns, 4);
}

GatherPlan new_plan(int kernel, bool bf16, int64_t items)
{
    GatherPlan p{};
    p.kernel = kernel; p.bf16 = bf16; p.k = 15; p.csplit = 1; p.grid = ws_grid(items, 4);
    return p;
}

// ws_kpconv_gather_fwd / _bf16 / _ex
int fwd_plan(bool bf16, int64_t nq, int32_t ci, const void* x, const void* wf, bool deformed, bool modulated, int32_t influence,
             int32_t aggregation, bool rows_sorted, GatherPlan& p)
{
    p = new_plan(ci > 4 ? GK_FWD_MFMA : GK_FWD_POOL, bf16, nq);
    p.def = deformed; p.rows_sorted = rows_sorted;
    if (int rc = rows_vec4_or_f32(bf16, ci, x, wf, p.vec)) return rc;
    if (ci > 4) {      // (the 3..4-channel input layer: the narrow-row pool form is 10 % faster)
        // matrix-core form (kpconv_gather_fwd_mfma_kernel): NT consecutive channels per lane, 16 NT channels per block
        const bool fastm = rigid_fast(deformed, modulated, influence, aggregation);
        p.n = nt_for_rows(ci, x, wf);
        p.mode = fastm ? 0 : 1; p.vec = true; p.cut = fastm && rows_sorted;
        if (fastm && !rows_sorted && nq < SPLIT_ROWS) {
            if (p.n > SPLIT_NT && ci % SPLIT_NT == 0) p.n = SPLIT_NT;       // narrower blocks: more items per query
            if (ci > 16 * p.n) {
                p.csplit = (ci + 16 * p.n - 1) / (16 * p.n);               // one channel block per item
                p.grid = ws_grid(nq * p.csplit, 4);
            }
        }
        return WS_OK;
    }
    // the 3..4-channel input layer: entry pool + VALU accumulate (kpconv_gather_fwd_kernel); rows that are not float4 (the
    // 3-channel input layer) in 4-byte pieces, 16 slots of 4 lanes
    p.mode = (!deformed && influence == WS_INFLUENCE_LINEAR && aggregation == WS_AGGREGATION_SUM) ? 0 : 1;
    p.n = p.vec ? 1 : 4; p.pw = p.vec ? 4 : 1;
    return WS_OK;
}

// ws_kpconv_gather_fwd_def: no narrowing, no csplit; bf16 rows move in pairs at least
int fwd_def_plan(bool bf16, int64_t nq, int32_t ci, const void* x, const void* wf, bool rows_sorted, GatherPlan& p)
{
    p = new_plan(GK_FWD_MFMA, bf16, nq);
    p.n = nt_for_rows(ci, x, wf);
    p.mode = 2; p.def = true; p.vec = true; p.cut = rows_sorted;
    if (bf16 && p.n == 1 && (ci % 2)) return ws_fail(WS_ERR_UNSUPPORTED, "bf16 rows need an even channel count (ci=%d)", ci);
    return WS_OK;
}

// ws_kpconv_gather_bwd_x / _bf16 / _gated (mode 0 = rigid_fast, else 1) and ws_kpconv_gather_bwd_x_def (mode 2)
int bwd_x_plan(bool bf16, int64_t ns, int32_t ci, const void* dwf, const void* dx, int mode, GatherPlan& p)
{
    p = new_plan(GK_BWD_X, bf16, ns);
    p.n = group_ladder(ci); p.mode = mode;
    return rows_vec4_or_f32(bf16, ci, dwf, dx, p.vec);
}

// ws_kpconv_gather_bwd_x_packed: four supports per wave (kpconv_gather_bwd_x_packed_kernel) where the form applies -- f32 rows in
// float4 pieces, rigid / linear / sum (mode 0), fewer queries than supports and at most PACK_MEAN_MAX incoming pairs per
// support on average; otherwise the plan of ws_kpconv_gather_bwd_x_gated.  ordered: the supports come through a point order
// (four consecutive entries of it make a quad); the plan does not depend on it.
int bwd_x_packed_plan(bool bf16, int64_t nq, int64_t ns, int32_t h, int32_t ci, const void* dwf, const void* dx, int mode, bool ordered,
                      GatherPlan& p)
{
    if (int rc = bwd_x_plan(bf16, ns, ci, dwf, dx, mode, p)) return rc;
    (void)ordered;
    if (bf16 || !p.vec || mode != 0 || nq >= ns || nq * (int64_t)h > (int64_t)PACK_MEAN_MAX * ns) return WS_OK;
    p.kernel = GK_BWD_X_PACKED;
    p.grid = ws_grid(ws_ceil_div(ns, 4), 4);
    return WS_OK;
}

// ws_kpconv_gather_bwd_geom / _bf16
int bwd_geom_plan(bool bf16, int64_t nq, int32_t ci, const void* x, const void* dwf, GatherPlan& p)
{
    p = new_plan(GK_BWD_GEOM, bf16, nq);
    p.mode = 1; p.vec = rows_vec4(bf16, ci, x, dwf);
    return WS_OK;
}

// ws_kpconv_gather_bwd_x_grid / _bf16 / _gated (mode 0 = rigid_fast, else 1)
int bwd_x_grid_plan(bool bf16, int64_t ns, int32_t ci, const void* dwf, const void* dx, int mode, bool ordered, GatherPlan& p)
{
    p = new_plan(GK_BWD_X_GRID, bf16, ns);
    p.n = group_ladder(ci); p.mode = mode; p.sort = ws_kpconv_grid_sorted != 0;
    grid_walk_plan(ns, ordered, p);
    return rows_vec4_or_f32(bf16, ci, dwf, dx, p.vec);
}

// ws_kpconv_gather_bwd_x_grid_wide: rigid (MODE 0) or the deformable fast path (MODE 2); NCH 64-channel chunks per item, G = 16 only
int bwd_x_gridw_plan(bool bf16, int64_t ns, int32_t ci, const void* dwf, const void* dx, bool deformed, bool ordered, GatherPlan& p)
{
    p = new_plan(GK_BWD_X_GRIDW, bf16, ns);
    p.n = group_ladder(ci); p.mode = deformed ? 2 : 0;
    p.nch = (p.n < 16 || ci <= 64) ? 1 : (ci <= 128 ? 2 : 4);
    grid_walk_plan(ns, ordered, p);
    return rows_vec4_or_f32(bf16, ci, dwf, dx, p.vec);
}

// ws_kpconv_gather_bwd_geom_def: CK 4-channel pieces per lane; up to 128 channels the accumulators stay in registers (AREG)
int bwd_geom_def_plan(bool bf16, int64_t nq, int32_t ci, const void* x, const void* dwf, bool rows_sorted, GatherPlan& p)
{
    p = new_plan(GK_BWD_GEOM_DEF, bf16, nq);
    if (ci % 16 != 0 || !aligned16(x) || !aligned16(dwf))
        return ws_fail(WS_ERR_UNSUPPORTED, "geometry backward on the matrix core needs ci %% 16 == 0 and 16-byte aligned rows (ci=%d)", ci);
    p.mode = 2; p.vec = true; p.cut = rows_sorted;
    p.areg = ci == 16 || ci == 32 || ci == 64 || ci == 128;
    p.n = p.areg ? ci / 4 : (ci % 128 == 0 ? 32 : (ci % 64 == 0 ? 16 : (ci % 32 == 0 ? 8 : 4)));
    return WS_OK;
}

// "kernel<template arguments> key=value ..." of a plan
void plan_text(const GatherPlan& p, char* out, size_t n)
{
    const char* t = p.bf16 ? "bf16" : "float";
    auto b = [](bool v) { return v ? "true" : "false"; };
    char ks[16] = "";                        // the matrix-core forward names its size only where it is not 15
    if (p.k != 15) snprintf(ks, sizeof ks, "K=%d, ", p.k);
    switch (p.kernel) {
    case GK_FWD_MFMA:
        snprintf(out, n, "kpconv_gather_fwd_mfma_kernel<%sNT=%d, MODE=%d, DEF=%s, VECROW=%s, T=%s, CUT=%s> grid=%d csplit=%d", ks, p.n, p.mode,
                 b(p.def), b(p.vec), t, b(p.cut), p.grid, p.csplit);
        break;
    case GK_FWD_POOL:
        snprintf(out, n, "kpconv_gather_fwd_kernel<K=%d, G=%d, MODE=%d, DEF=%s, VEC=%s, PW=%d, T=%s> grid=%d csplit=%d cut=%d", p.k, p.n, p.mode,
                 b(p.def), b(p.vec), p.pw, t, p.grid, p.csplit, p.rows_sorted);
        break;
    case GK_BWD_X:
        snprintf(out, n, "kpconv_gather_bwd_x_kernel<K=%d, G=%d, MODE=%d, VEC=%s, T=%s> grid=%d", p.k, p.n, p.mode, b(p.vec), t, p.grid);
        break;
    case GK_BWD_X_PACKED:
        snprintf(out, n, "kpconv_gather_bwd_x_packed_kernel<K=%d, G=%d, VEC=%s, T=%s> grid=%d", p.k, p.n, b(p.vec), t, p.grid);
        break;
    case GK_BWD_GEOM:
        snprintf(out, n, "kpconv_gather_bwd_geom_kernel<K=%d, T=%s> grid=%d vec4=%d", p.k, t, p.grid, p.vec ? 1 : 0);
        break;
    case GK_BWD_X_GRID:
        snprintf(out, n, "kpconv_gather_bwd_x_grid_kernel<K=%d, G=%d, MODE=%d, VEC=%s, T=%s, SORT=%s> grid=%d ilv=%d", p.k, p.n, p.mode, b(p.vec),
                 t, b(p.sort), p.grid, p.ilv);
        break;
    case GK_BWD_X_GRIDW:
        snprintf(out, n, "kpconv_gather_bwd_x_gridw_kernel<K=%d, G=%d, MODE=%d, VEC=%s, NCH=%d, T=%s> grid=%d ilv=%d", p.k, p.n, p.mode,
                 b(p.vec), p.nch, t, p.grid, p.ilv);
        break;
    default:
        snprintf(out, n, "kpconv_gather_bwd_geom_def_kernel<CK=%d, AREG=%s, T=%s, CUT=%s> grid=%d", p.n, b(p.areg), t, b(p.cut), p.grid);
    }
}

int launched() { WS_LAUNCH_CHECK(); return WS_OK; }      // the end of every launcher

// ---- launchers: validate, plan, one launch_* call on the plan (kpconv_launch.h) ------------------------------------------
// packed: the plan of ws_kpconv_gather_bwd_x_packed (f32 rows) instead of bwd_x_plan
int gather_bwd_x_impl(bool bf16, const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, int32_t h, const int32_t* t_offsets,
                      const int32_t* t_pairs, const void* dwf, int32_t ci, const float* kernel_points, int32_t k, const float* deformed_kp,
                      const float* modulations, float extent, int32_t influence, int32_t aggregation, const int32_t* order, void* dx,
                      void* stream, const void* gate = nullptr, float gate_slope = 0.0f, bool packed = false)
{
    if (int rc = check_common(q_pts, nq, s_pts, ns, h, ci, k, extent, influence, aggregation)) return rc;
    if (ns == 0) return WS_OK;
    WS_REQUIRE(t_offsets && t_pairs && dwf && dx && (kernel_points || deformed_kp), "NULL argument");
    WS_REQUIRE(nq * (int64_t)h < (1ll << 31), "nq*h exceeds int32");
    WS_REQUIRE(nq * (int64_t)k * ci < (1ll << 31), "nq*k*ci exceeds the 32-bit row offsets of the gather");
    GatherPlan p;
    const int mode = rigid_fast(deformed_kp, modulations, influence, aggregation) ? 0 : 1;
    if (int rc = check_k(k, bf16, mode)) return rc;
    if (int rc = packed ? bwd_x_packed_plan(bf16, nq, ns, h, ci, dwf, dx, mode, order != nullptr, p) : bwd_x_plan(bf16, ns, ci, dwf, dx, mode, p))
        return rc;
    p.k = k;
    GeomParams g{extent, influence, aggregation, deformed_kp ? 1 : 0, gate, gate_slope, nullptr, 0};
    if (p.kernel == GK_BWD_X_PACKED) {
        launch_bwd_x_packed(p, stream, q_pts, nq, s_pts, ns, h, t_offsets, t_pairs, (const float*)dwf, ci, kernel_points, g, (float*)dx, order);
        return launched();
    }
    launch_bwd_x(p, stream, q_pts, nq, s_pts, ns, h, t_offsets, t_pairs, dwf, ci, kernel_points, deformed_kp, modulations, g, dx, order);
    return launched();
}

int gather_bwd_geom_impl(bool bf16, const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int64_t* inds, int32_t h,
                         const void* x, int32_t ci, const void* dwf, int32_t k, const float* deformed_kp, const float* modulations,
                         const float* d_min_d2, float extent, int32_t influence, int32_t aggregation, float* d_deformed_kp,
                         float* d_modulations, void* stream)
{
    if (int rc = check_common(q_pts, nq, s_pts, ns, h, ci, k, extent, influence, aggregation)) return rc;
    if (nq == 0) return WS_OK;
    WS_REQUIRE(inds && x && dwf && deformed_kp && d_deformed_kp, "NULL argument");
    GatherPlan p;
    if (int rc = check_k(k, bf16, 1)) return rc;
    if (int rc = bwd_geom_plan(bf16, nq, ci, x, dwf, p)) return rc;
    p.k = k;
    GeomParams g{extent, influence, aggregation, 1, nullptr, 0.0f, nullptr, 0};
    launch_bwd_geom(p, stream, q_pts, nq, s_pts, ns, inds, h, x, ci, dwf, deformed_kp, modulations, d_min_d2, g, d_deformed_kp, d_modulations);
    return launched();
}

int gather_bwd_x_grid_impl(bool bf16, const float* s_pts, int64_t ns, const void* grid_blob, int32_t nb, int64_t cells,
                           const uint64_t* key_last, float radius, const void* dwf, int32_t ci, const float* kernel_points, int32_t k,
                           const float* deformed_kp, const float* modulations, float extent, int32_t influence, int32_t aggregation,
                           const int32_t* order, void* dx, int32_t* overflow, void* stream, const void* gate = nullptr,
                           float gate_slope = 0.0f, const int64_t* rows = nullptr, int32_t rows_h = 0)
{
    if (int rc = check_common(s_pts, ns, s_pts, ns, 1, ci, k, extent, influence, aggregation)) return rc;
    if (ns == 0) return WS_OK;
    WS_REQUIRE(grid_blob && key_last && dwf && dx && overflow && (kernel_points || deformed_kp), "NULL argument");
    WS_REQUIRE(nb >= 1 && cells >= 1, "bad grid nb=%d cells=%lld", nb, (long long)cells);
    WS_REQUIRE(ns * (int64_t)k * ci < (1ll << 31), "ns*k*ci exceeds the 32-bit row offsets of the gather");
    WS_REQUIRE(!rows || rows_h >= 1, "index rows given without their width");
    GatherPlan p;
    const int mode = rigid_fast(deformed_kp, modulations, influence, aggregation) ? 0 : 1;
    if (int rc = check_k(k, bf16, mode)) return rc;
    if (int rc = bwd_x_grid_plan(bf16, ns, ci, dwf, dx, mode, order != nullptr, p)) return rc;
    p.k = k;
    GeomParams g{extent, influence, aggregation, deformed_kp ? 1 : 0, gate, gate_slope, rows, rows_h, nullptr, nullptr, 0, p.ilv};
    const GridView v = grid_view(grid_blob, nb, cells, key_last, radius);
    launch_bwd_x_grid(p, stream, s_pts, ns, v, nb, dwf, ci, kernel_points, deformed_kp, modulations, g, dx, order, overflow);
    return launched();
}

}  // namespace

extern "C" {

// ws_kpconv_gather_fwd / _bf16 for index rows that are sorted by distance from their query (rows_sorted != 0: what the radius
// search delivers): the rigid linear / sum forms then stop at the reach of the kernel points (see CUT in kpconv_fwd.hip); other
// modes and rows_sorted == 0 are the plain entries.
int ws_kpconv_gather_fwd_ex(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int64_t* inds, int32_t h,
                            const void* x, int32_t ci, const float* kernel_points, int32_t k, const float* deformed_kp,
                            const float* modulations, float extent, int32_t influence, int32_t aggregation, const int32_t* order,
                            void* wf, float* min_d2, int32_t rows_bf16, int32_t rows_sorted, void* stream)
{
    if (int rc = check_common(q_pts, nq, s_pts, ns, h, ci, k, extent, influence, aggregation)) return rc;
    if (nq == 0) return WS_OK;
    WS_REQUIRE(inds && x && wf && (kernel_points || deformed_kp), "NULL argument");
    WS_REQUIRE(ns * (int64_t)ci < (1ll << 31), "ns*ci exceeds the 32-bit row offsets of the gather");
    GatherPlan p;
    if (int rc = check_k(k, rows_bf16 != 0, 0)) return rc;
    if (int rc = fwd_plan(rows_bf16 != 0, nq, ci, x, wf, deformed_kp, modulations, influence, aggregation, rows_sorted != 0, p)) return rc;
    p.k = k;
    GeomParams g{extent, influence, aggregation, deformed_kp ? 1 : 0, nullptr, 0.0f, nullptr, 0, nullptr, nullptr, p.rows_sorted, 0, p.csplit};
    if (p.kernel == GK_FWD_MFMA)
        launch_fwd_mfma(p, stream, q_pts, nq, s_pts, ns, inds, h, x, ci, kernel_points, deformed_kp, modulations, g, wf, min_d2, order);
    else
        launch_fwd_pool(p, stream, q_pts, nq, s_pts, ns, inds, h, x, ci, kernel_points, deformed_kp, modulations, g, wf, min_d2, order);
    return launched();
}

int ws_kpconv_gather_fwd(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns,
                         const int64_t* inds, int32_t h, const float* x, int32_t ci,
                         const float* kernel_points, int32_t k, const float* deformed_kp,
                         const float* modulations, float extent, int32_t influence, int32_t aggregation,
                         const int32_t* order, float* wf, float* min_d2, void* stream)
{
    return ws_kpconv_gather_fwd_ex(q_pts, nq, s_pts, ns, inds, h, x, ci, kernel_points, k, deformed_kp, modulations, extent, influence,
                                   aggregation, order, wf, min_d2, 0, 0, stream);
}

int ws_kpconv_gather_fwd_bf16(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns,
                              const int64_t* inds, int32_t h, const uint16_t* x, int32_t ci,
                              const float* kernel_points, int32_t k, const float* deformed_kp,
                              const float* modulations, float extent, int32_t influence, int32_t aggregation,
                              const int32_t* order, uint16_t* wf, float* min_d2, void* stream)
{
    return ws_kpconv_gather_fwd_ex(q_pts, nq, s_pts, ns, inds, h, x, ci, kernel_points, k, deformed_kp, modulations, extent, influence,
                                   aggregation, order, wf, min_d2, 1, 0, stream);
}

// ---- deformable fast path: deformable (+ modulated) KPConv with linear influence and sum aggregation, the per-query kernel
//      points packed as kp4 [nq, 15] float4 (x, y, z, modulation; ws_kpconv_deform_prepare).  rows_bf16: feature rows
//      (x, wf, dwf, dx) are bf16 instead of f32.
int ws_kpconv_gather_fwd_def(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int64_t* inds, int32_t h,
                             const void* x, int32_t ci, const float* kp4, int32_t k, float extent, const int32_t* order,
                             void* wf, float* min_d2, int32_t rows_bf16, int32_t rows_sorted, void* stream)
{
    if (int rc = check_common(q_pts, nq, s_pts, ns, h, ci, k, extent, WS_INFLUENCE_LINEAR, WS_AGGREGATION_SUM)) return rc;
    if (nq == 0) return WS_OK;
    WS_REQUIRE(inds && x && wf && kp4, "NULL argument");
    WS_REQUIRE(aligned16(kp4), "kp4 must be 16-byte aligned");
    WS_REQUIRE(ns * (int64_t)ci < (1ll << 31), "ns*ci exceeds the 32-bit row offsets of the gather");
    GatherPlan p;
    if (int rc = check_k(k, rows_bf16 != 0, 2)) return rc;
    if (int rc = fwd_def_plan(rows_bf16 != 0, nq, ci, x, wf, rows_sorted != 0, p)) return rc;
    GeomParams g{extent, WS_INFLUENCE_LINEAR, WS_AGGREGATION_SUM, 1, nullptr, 0.0f, nullptr, 0, reinterpret_cast<const float4*>(kp4)};
    launch_fwd_mfma(p, stream, q_pts, nq, s_pts, ns, inds, h, x, ci, nullptr, nullptr, nullptr, g, wf, min_d2, order);
    return launched();
}

int ws_kpconv_gather_bwd_x_def(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, int32_t h,
                               const int32_t* t_offsets, const int32_t* t_pairs, const void* dwf, int32_t ci, const float* kp4,
                               int32_t k, float extent, const int32_t* order, void* dx, int32_t rows_bf16, void* stream)
{
    if (int rc = check_common(q_pts, nq, s_pts, ns, h, ci, k, extent, WS_INFLUENCE_LINEAR, WS_AGGREGATION_SUM)) return rc;
    if (ns == 0) return WS_OK;
    WS_REQUIRE(t_offsets && t_pairs && dwf && dx && kp4 && aligned16(kp4), "NULL / unaligned argument");
    WS_REQUIRE(nq * (int64_t)h < (1ll << 31), "nq*h exceeds int32");
    WS_REQUIRE(nq * (int64_t)k * ci < (1ll << 31), "nq*k*ci exceeds the 32-bit row offsets of the gather");
    GatherPlan p;
    if (int rc = check_k(k, rows_bf16 != 0, 2)) return rc;
    if (int rc = bwd_x_plan(rows_bf16 != 0, ns, ci, dwf, dx, 2, p)) return rc;
    GeomParams g{extent, WS_INFLUENCE_LINEAR, WS_AGGREGATION_SUM, 1, nullptr, 0.0f, nullptr, 0, reinterpret_cast<const float4*>(kp4)};
    launch_bwd_x(p, stream, q_pts, nq, s_pts, ns, h, t_offsets, t_pairs, dwf, ci, nullptr, nullptr, nullptr, g, dx, order);
    return launched();
}

// the table-free backward for any in-degree (rows wider than 128): rigid (kp4 NULL, kernel_points given) or deformable (kp4)
int ws_kpconv_gather_bwd_x_grid_wide(const float* s_pts, int64_t ns, const void* grid_blob, int32_t nb, int64_t cells,
                                     const uint64_t* key_last, float radius, const void* dwf, int32_t ci,
                                     const float* kernel_points, int32_t k, const float* kp4, const float* kp_rmax, float extent,
                                     const int32_t* order, const int64_t* rows, int32_t rows_h, void* dx, int32_t rows_bf16,
                                     void* stream)
{
    if (int rc = check_common(s_pts, ns, s_pts, ns, 1, ci, k, extent, WS_INFLUENCE_LINEAR, WS_AGGREGATION_SUM)) return rc;
    if (ns == 0) return WS_OK;
    WS_REQUIRE(grid_blob && key_last && dwf && dx && (kernel_points || kp4), "NULL argument");
    WS_REQUIRE(!kp4 || aligned16(kp4), "kp4 must be 16-byte aligned");
    WS_REQUIRE(nb >= 1 && cells >= 1, "bad grid nb=%d cells=%lld", nb, (long long)cells);
    WS_REQUIRE(ns * (int64_t)k * ci < (1ll << 31), "ns*k*ci exceeds the 32-bit row offsets of the gather");
    WS_REQUIRE(!rows || rows_h >= 1, "index rows given without their width");
    GatherPlan p;
    if (int rc = check_k(k, rows_bf16 != 0, kp4 ? 2 : 0)) return rc;
    if (int rc = bwd_x_gridw_plan(rows_bf16 != 0, ns, ci, dwf, dx, kp4 != nullptr, order != nullptr, p)) return rc;
    p.k = k;
    // no kp_rmax from the caller: the entry takes the maximum itself, so the candidates -- and with them the 64-pair batches and
    // the association of the sums -- do not depend on whether the caller kept the scalar.  The word is stream-ordered memory of
    // this call (freed on every way out); not under a stream capture, where the allocation would become a node of the graph:
    // a captured caller passes kp_rmax.  (The helper launch is not counted: ws_launch_count counts the entry's one launch.)
    struct OwnWord {
        float* p = nullptr;
        hipStream_t st;
        ~OwnWord() { if (p) (void)hipFreeAsync(p, st); }
    } own{nullptr, (hipStream_t)stream};
    if (kp4 && !kp_rmax) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        WS_HIP(hipStreamIsCapturing(own.st, &cap));
        if (cap != hipStreamCaptureStatusNone)
            return ws_fail(WS_ERR_UNSUPPORTED, "deformable grid backward under a stream capture needs kp_rmax from the caller");
        WS_HIP(hipMallocAsync((void**)&own.p, sizeof(float), own.st));
        WS_HIP(hipMemsetAsync(own.p, 0, sizeof(float), own.st));
        launch_kp4_rmax(own.st, kp4, ns * (int64_t)k, own.p);
        WS_HIP(hipGetLastError());
        kp_rmax = own.p;
    }
    GeomParams g{extent, WS_INFLUENCE_LINEAR, WS_AGGREGATION_SUM, kp4 ? 1 : 0, nullptr, 0.0f, rows, rows_h,
                 reinterpret_cast<const float4*>(kp4), kp4 ? kp_rmax : nullptr, 0, p.ilv};
    const GridView v = grid_view(grid_blob, nb, cells, key_last, radius);
    launch_bwd_x_gridw(p, stream, s_pts, ns, v, nb, dwf, ci, kernel_points, g, dx, order);
    return launched();
}

int ws_kpconv_gather_bwd_geom_def(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int64_t* inds, int32_t h,
                                  const void* x, int32_t ci, const void* dwf, const float* kp4, int32_t k, const float* d_min_d2,
                                  float extent, const int32_t* order, float* d_kp4, int32_t rows_bf16, int32_t rows_sorted,
                                  void* stream)
{
    if (int rc = check_common(q_pts, nq, s_pts, ns, h, ci, k, extent, WS_INFLUENCE_LINEAR, WS_AGGREGATION_SUM)) return rc;
    if (nq == 0) return WS_OK;
    WS_REQUIRE(inds && x && dwf && kp4 && d_kp4 && aligned16(kp4) && aligned16(d_kp4), "NULL / unaligned argument");
    WS_REQUIRE(ns * (int64_t)ci < (1ll << 31) && nq * (int64_t)k * ci < (1ll << 31), "row offsets exceed 32 bits");
    GatherPlan p;
    if (int rc = check_k(k, rows_bf16 != 0, 2)) return rc;
    if (int rc = bwd_geom_def_plan(rows_bf16 != 0, nq, ci, x, dwf, rows_sorted != 0, p)) return rc;
    launch_bwd_geom_def(p, stream, q_pts, nq, s_pts, ns, inds, h, x, ci, dwf, kp4, d_min_d2, extent, d_kp4, order);
    return launched();
}

// Forward-only KPConv layer in ONE launch (inference: the testers' forward passes, utils/tester_PseudoLabel.py:164):
// out = act(KPConv(x) + bias) for rigid / linear / sum layers of 32 -> 32 f32 channels -- the level-0 layers of the DALES
// networks, where `wf` is largest (kpconv_gather_fwd_mfma_kernel<..., FUSE>).  Other shapes: WS_ERR_UNSUPPORTED (the caller
// runs gather + contraction as two launches).
int ws_kpconv_layer_fwd_fused(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int64_t* inds, int32_t h,
                              const float* x, int32_t ci, const float* kernel_points, int32_t k, float extent,
                              const int32_t* order, const float* weights, int32_t co, const float* bias, int32_t act, float slope,
                              float* out, void* stream)
{
    int rc = check_common(q_pts, nq, s_pts, ns, h, ci, k, extent, WS_INFLUENCE_LINEAR, WS_AGGREGATION_SUM);
    if (rc) return rc;
    if (k != 15) return ws_fail(WS_ERR_UNSUPPORTED, "num_kernel_points=%d: the fused forward layer is built for K=15 only (of K=9, K=13 and K=15)", k);
    if (ci != 32 || co != 32 || !aligned16(x) || !aligned16(weights) || !aligned16(out))
        return ws_fail(WS_ERR_UNSUPPORTED, "fused forward layer: 32 -> 32 channels, 16-byte aligned rows (got %d -> %d)", ci, co);
    if (nq == 0) return WS_OK;
    WS_REQUIRE(inds && x && kernel_points && weights && out, "NULL argument");
    WS_REQUIRE(ns * (int64_t)ci < (1ll << 31), "ns*ci exceeds the 32-bit row offsets of the gather");
    GeomParams g{extent, WS_INFLUENCE_LINEAR, WS_AGGREGATION_SUM, 0, nullptr, 0.0f, nullptr, 0, nullptr, nullptr, 0};
    FuseArgs fz{weights, bias, slope, act, out};
    launch_fwd_fused(stream, q_pts, nq, s_pts, ns, inds, h, x, ci, kernel_points, g, order, fz);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

// What the launchers of this file launch for these arguments, as "kernel<template arguments> key=value ..." (grid, csplit, ilv):
// the plan function of the entry named by op (WS_GATHER_*, weasal_hip.h), nothing read or launched.  rows_a / rows_b: the two
// feature-row operands of that entry (x and wf, dwf and dx, or x and dwf), tested for alignment only.
int ws_kpconv_gather_variant(int32_t op, int64_t nq, int64_t ns, int32_t ci, const void* rows_a, const void* rows_b, int32_t deformed,
                             int32_t modulated, int32_t influence, int32_t aggregation, int32_t rows_bf16, int32_t rows_sorted,
                             int32_t ordered, char* out, int32_t cap)
{
    return ws_kpconv_gather_variant_k(op, nq, ns, ci, rows_a, rows_b, deformed, modulated, influence, aggregation, rows_bf16, rows_sorted,
                                      ordered, 15, out, cap);
}

// 1 where the gather entries run k kernel points with these rows (rows_bf16) in this MODE (0 rigid / linear / sum, 1 the generic
// form, 2 the deformable fast path with packed kernel points), else 0: what the Python layers ask instead of comparing with 15
int ws_kpconv_supported_k(int32_t k, int32_t rows_bf16, int32_t mode)
{
    return (mode >= 0 && mode <= 2 && supported_k(k, rows_bf16 != 0, mode)) ? 1 : 0;
}

// ws_kpconv_gather_variant for k kernel points: the same text with the size in it (K=13 where the kernel has a K field, a
// leading "K=13, " in the matrix-core forward's list; k = 15 prints what ws_kpconv_gather_variant always printed); a size
// or form this build does not have is refused like the entry refuses it
int ws_kpconv_gather_variant_k(int32_t op, int64_t nq, int64_t ns, int32_t ci, const void* rows_a, const void* rows_b, int32_t deformed,
                               int32_t modulated, int32_t influence, int32_t aggregation, int32_t rows_bf16, int32_t rows_sorted,
                               int32_t ordered, int32_t k, char* out, int32_t cap)
{
    WS_REQUIRE(out && cap > 0 && ci >= 1 && nq >= 0 && ns >= 0, "bad argument");
    const bool bf = rows_bf16 != 0, def = deformed != 0, mod = modulated != 0, srt = rows_sorted != 0, ord = ordered != 0;
    const int mode = rigid_fast(def, mod, influence, aggregation) ? 0 : 1;
    GatherPlan p;
    int rc;
    switch (op) {
    case WS_GATHER_FWD: rc = fwd_plan(bf, nq, ci, rows_a, rows_b, def, mod, influence, aggregation, srt, p); break;
    case WS_GATHER_BWD_X: rc = bwd_x_plan(bf, ns, ci, rows_a, rows_b, mode, p); break;
    case WS_GATHER_BWD_GEOM: rc = bwd_geom_plan(bf, nq, ci, rows_a, rows_b, p); break;
    case WS_GATHER_BWD_X_GRID: rc = bwd_x_grid_plan(bf, ns, ci, rows_a, rows_b, mode, ord, p); break;
    case WS_GATHER_FWD_DEF: rc = fwd_def_plan(bf, nq, ci, rows_a, rows_b, srt, p); break;
    case WS_GATHER_BWD_X_DEF: rc = bwd_x_plan(bf, ns, ci, rows_a, rows_b, 2, p); break;
    case WS_GATHER_BWD_X_GRID_WIDE: rc = bwd_x_gridw_plan(bf, ns, ci, rows_a, rows_b, def, ord, p); break;
    case WS_GATHER_BWD_GEOM_DEF: rc = bwd_geom_def_plan(bf, nq, ci, rows_a, rows_b, srt, p); break;
    default: return ws_fail(WS_ERR_INVALID, "unknown gather operation %d", op);
    }
    if (rc != WS_OK) return rc;
    if (int rk = check_k(k, bf, p.mode)) return rk;
    p.k = k;
    plan_text(p, out, (size_t)cap);
    return WS_OK;
}

// Name of the forward gather kernel a layer launches (bench.py's roofline.kernel): the forward plan for 16-byte aligned rows at
// nq = SPLIT_ROWS (a level too large for the SPLIT_NT narrowing and csplit), in the form this entry has always printed.  mode: 0 rigid
// (kernel_points), 1 deformable through the generic entries, 2 deformable fast path (kp4).
int ws_kpconv_gather_fwd_variant(int32_t ci, int32_t mode, int32_t influence, int32_t aggregation, int32_t rows_bf16,
                                 int32_t rows_sorted, char* out, int32_t cap)
{
    WS_REQUIRE(out && cap > 0 && ci >= 1, "bad argument");
    alignas(16) static const char row[16] = {};
    const bool bf = rows_bf16 != 0, srt = rows_sorted != 0;
    GatherPlan p;
    if (int rc = mode == 2 ? fwd_def_plan(bf, SPLIT_ROWS, ci, row, row, srt, p)
                           : fwd_plan(bf, SPLIT_ROWS, ci, row, row, mode != 0, false, influence, aggregation, srt, p))
        return rc;
    const char* t = bf ? "bf16" : "float";
    auto b = [](bool v) { return v ? "true" : "false"; };
    if (p.kernel == GK_FWD_MFMA)
        snprintf(out, (size_t)cap, "kpconv_gather_fwd_mfma_kernel<NT=%d, MODE=%d, DEF=%s, VECROW=true, %s, GS=default, CUT=%s>", p.n, p.mode,
                 b(p.def), t, b(p.cut));
    else
        snprintf(out, (size_t)cap, "kpconv_gather_fwd_kernel<K=15, G=%d, MODE=%d, DEF=%s, VEC=%s, PW=%d, %s>%s", p.n, p.mode, b(p.def),
                 b(p.vec), p.pw, t, (p.rows_sorted && p.mode == 0) ? " (sorted-row cutoff on)" : "");
    return WS_OK;
}

int ws_kpconv_gather_bwd_x(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns,
                           const int64_t* inds, int32_t h, const int32_t* t_offsets, const int32_t* t_pairs,
                           const float* dwf, int32_t ci, const float* kernel_points, int32_t k,
                           const float* deformed_kp, const float* modulations, float extent,
                           int32_t influence, int32_t aggregation, const int32_t* order, float* dx, void* stream)
{
    return gather_bwd_x_impl(false, q_pts, nq, s_pts, ns, h, t_offsets, t_pairs, dwf, ci, kernel_points, k, deformed_kp, modulations, extent,
                             influence, aggregation, order, dx, stream);
}

int ws_kpconv_gather_bwd_x_bf16(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns,
                                const int64_t* inds, int32_t h, const int32_t* t_offsets, const int32_t* t_pairs,
                                const uint16_t* dwf, int32_t ci, const float* kernel_points, int32_t k,
                                const float* deformed_kp, const float* modulations, float extent,
                                int32_t influence, int32_t aggregation, const int32_t* order, uint16_t* dx, void* stream)
{
    return gather_bwd_x_impl(true, q_pts, nq, s_pts, ns, h, t_offsets, t_pairs, dwf, ci, kernel_points, k, deformed_kp, modulations, extent,
                             influence, aggregation, order, dx, stream);
}

int ws_kpconv_gather_bwd_geom(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns,
                              const int64_t* inds, int32_t h, const float* x, int32_t ci, const float* dwf,
                              const float* kernel_points, int32_t k, const float* deformed_kp,
                              const float* modulations, const float* d_min_d2, float extent,
                              int32_t influence, int32_t aggregation, float* d_deformed_kp,
                              float* d_modulations, void* stream)
{
    return gather_bwd_geom_impl(false, q_pts, nq, s_pts, ns, inds, h, x, ci, dwf, k, deformed_kp, modulations, d_min_d2, extent, influence,
                                aggregation, d_deformed_kp, d_modulations, stream);
}

int ws_kpconv_gather_bwd_geom_bf16(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns,
                                   const int64_t* inds, int32_t h, const uint16_t* x, int32_t ci, const uint16_t* dwf,
                                   const float* kernel_points, int32_t k, const float* deformed_kp,
                                   const float* modulations, const float* d_min_d2, float extent,
                                   int32_t influence, int32_t aggregation, float* d_deformed_kp,
                                   float* d_modulations, void* stream)
{
    return gather_bwd_geom_impl(true, q_pts, nq, s_pts, ns, inds, h, x, ci, dwf, k, deformed_kp, modulations, d_min_d2, extent, influence,
                                aggregation, d_deformed_kp, d_modulations, stream);
}

int ws_kpconv_gather_bwd_x_grid(const float* s_pts, int64_t ns, const void* grid_blob, int32_t nb, int64_t cells,
                                const uint64_t* key_last, float radius, const float* dwf, int32_t ci,
                                const float* kernel_points, int32_t k, const float* deformed_kp, const float* modulations,
                                float extent, int32_t influence, int32_t aggregation, const int32_t* order, float* dx,
                                int32_t* overflow, void* stream)
{
    return gather_bwd_x_grid_impl(false, s_pts, ns, grid_blob, nb, cells, key_last, radius, dwf, ci, kernel_points, k, deformed_kp,
                                  modulations, extent, influence, aggregation, order, dx, overflow, stream);
}

int ws_kpconv_gather_bwd_x_grid_bf16(const float* s_pts, int64_t ns, const void* grid_blob, int32_t nb, int64_t cells,
                                     const uint64_t* key_last, float radius, const uint16_t* dwf, int32_t ci,
                                     const float* kernel_points, int32_t k, const float* deformed_kp, const float* modulations,
                                     float extent, int32_t influence, int32_t aggregation, const int32_t* order, uint16_t* dx,
                                     int32_t* overflow, void* stream)
{
    return gather_bwd_x_grid_impl(true, s_pts, ns, grid_blob, nb, cells, key_last, radius, dwf, ci, kernel_points, k, deformed_kp,
                                  modulations, extent, influence, aggregation, order, dx, overflow, stream);
}

// K4 / K4G with the activation backward of the preceding unary block folded into the store: dx * LeakyReLU'(gate_y)
// (gate_y [ns, ci] = that block's activated output, i.e. this layer's input x).  gate_y NULL = the plain entries above.
int ws_kpconv_gather_bwd_x_gated(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns,
                                 const int64_t* inds, int32_t h, const int32_t* t_offsets, const int32_t* t_pairs,
                                 const float* dwf, int32_t ci, const float* kernel_points, int32_t k,
                                 const float* deformed_kp, const float* modulations, float extent,
                                 int32_t influence, int32_t aggregation, const int32_t* order, const float* gate_y,
                                 float gate_slope, float* dx, void* stream)
{
    return gather_bwd_x_impl(false, q_pts, nq, s_pts, ns, h, t_offsets, t_pairs, dwf, ci, kernel_points, k, deformed_kp, modulations, extent,
                             influence, aggregation, order, dx, stream, gate_y, gate_slope);
}

// ws_kpconv_gather_bwd_x_gated with four supports per wave where that form applies (bwd_x_packed_plan): the same dx, bit for bit
int ws_kpconv_gather_bwd_x_packed(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns,
                                  const int64_t* inds, int32_t h, const int32_t* t_offsets, const int32_t* t_pairs,
                                  const float* dwf, int32_t ci, const float* kernel_points, int32_t k,
                                  const float* deformed_kp, const float* modulations, float extent,
                                  int32_t influence, int32_t aggregation, const int32_t* order, const float* gate_y,
                                  float gate_slope, float* dx, void* stream)
{
    return gather_bwd_x_impl(false, q_pts, nq, s_pts, ns, h, t_offsets, t_pairs, dwf, ci, kernel_points, k, deformed_kp, modulations, extent,
                             influence, aggregation, order, dx, stream, gate_y, gate_slope, true);
}

// What ws_kpconv_gather_bwd_x_packed launches for these arguments (dwf / dx: their alignment only): the packed kernel and its
// template arguments, or "none" -- the entry then launches what ws_kpconv_gather_bwd_x_gated launches (ws_kpconv_gather_variant,
// WS_GATHER_BWD_X).  bf16 rows have no packed entry: "none".
int ws_kpconv_gather_bwd_x_packed_variant(int64_t nq, int64_t ns, int32_t h, int32_t ci, const void* dwf, const void* dx, int32_t deformed,
                                          int32_t modulated, int32_t influence, int32_t aggregation, int32_t rows_bf16, int32_t ordered,
                                          char* out, int32_t cap)
{
    WS_REQUIRE(out && cap > 0 && ci >= 1 && h >= 1 && nq >= 0 && ns >= 0, "bad argument");
    GatherPlan p;
    const int mode = rigid_fast(deformed != 0, modulated != 0, influence, aggregation) ? 0 : 1;
    if (int rc = bwd_x_packed_plan(rows_bf16 != 0, nq, ns, h, ci, dwf, dx, mode, ordered != 0, p)) return rc;
    if (p.kernel == GK_BWD_X_PACKED) plan_text(p, out, (size_t)cap);
    else snprintf(out, (size_t)cap, "none");
    return WS_OK;
}

int ws_kpconv_gather_bwd_x_grid_gated(const float* s_pts, int64_t ns, const void* grid_blob, int32_t nb, int64_t cells,
                                      const uint64_t* key_last, float radius, const float* dwf, int32_t ci,
                                      const float* kernel_points, int32_t k, const float* deformed_kp, const float* modulations,
                                      float extent, int32_t influence, int32_t aggregation, const int32_t* order,
                                      const float* gate_y, float gate_slope, const int64_t* rows, int32_t rows_h, float* dx,
                                      int32_t* overflow, void* stream)
{
    return gather_bwd_x_grid_impl(false, s_pts, ns, grid_blob, nb, cells, key_last, radius, dwf, ci, kernel_points, k, deformed_kp,
                                  modulations, extent, influence, aggregation, order, dx, overflow, stream, gate_y, gate_slope, rows, rows_h);
}

}  // extern "C"
