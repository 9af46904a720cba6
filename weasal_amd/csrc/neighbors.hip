// weasal_amd/csrc/neighbors.hip -- batched fixed-radius neighbour search on gfx950.
// (compiled with -ffp-contract=off: the distance recipe must round like the reference's, no FMA)
//
// Replaces batch_nanoflann_neighbors (cpp_wrappers/cpp_neighbors/neighbors/neighbors.cpp:211-332):
// the kd-tree + per-query std::sort become
//   1. per batch element: bounding box -> uniform cell grid (cell slightly > radius), supports
//      counting-sorted by cell (x-fastest), stored as float4 (x,y,z,index) so that a run of cells
//      is one contiguous, coalesced segment;
//   2. one wave per query: the 3x3x3 cell block is 9 contiguous runs; 64 lanes test 64 candidates
//      per step with the reference's exact f32 recipe  ((dx*dx + dy*dy) + dz*dz) < r*r,
//      wave ballot + popcount-prefix compacts the hits into the wave's LDS slab;
//   3. the slab is sorted on the 64-bit (distance, index) key (nb_key, ws_grid.h) and written as one row.
// Pass A (plan) only counts (-> max_count, the data-dependent width, neighbors.cpp:296-304),
// pass B (fill) sorts and writes int32 or int64 rows padded with ns (neighbors.cpp:324).
// The kernels are in neighbors_kernels.h (the walk they share with the grid-walk KPConv backward: ws_grid.h); here the
// workspace, the fill plan (nb_fill_plan) and the entries.  The exact nearest-neighbour search without a radius
// (ws_nearest_neighbors, kernels in nearest_kernels.h) walks the same grid and is the last entry of this file.
#include "neighbors_kernels.h"
#include "nearest_kernels.h"
#include "ws_dispatch.h"
#include <vector>
#include <algorithm>

namespace {

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    int ensure(size_t n)
    {
        if (n <= cap) return WS_OK;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        size_t want = n + n / 4 + 64;
        WS_HIP(hipMalloc((void**)&p, want * sizeof(T)));
        cap = want;
        return WS_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

}  // namespace

struct ws_neighbors_ws {
    DevBuf<CloudGrid> grids;
    DevBuf<float> bbox;
    DevBuf<int32_t> cell_of, cell_start, cursor, counts, scan_scratch, max_count;
    DevBuf<float4> sorted, sorted_alt;      // (sorted_alt: the arrival-ordered copy the bin fill writes; see nb_cell_rank_kernel)
    DevBuf<int32_t> order;        // supports in cell order (work order of self-queries)
    bool self_query = false;      // queries == supports: walk the queries in cell order
    // state of the last plan
    const float* queries = nullptr;
    int64_t nq = 0, ns = 0;
    int nb = 0;
    float r2 = 0.f;
    int max_count_host = 0;
    int64_t cells = 0;                         // cells of the last plan (all elements)
    int32_t* max_count_word = nullptr;         // device word holding the maximum row length of the current plan
    unsigned long long* key_last = nullptr;    // one-shot output of the next fill (ws_radius_neighbors_set_key_last)
    bool reuse_next = false;                   // one-shot: the next plan keeps the support grid (ws_radius_neighbors_reuse_grid)
    const float* supports = nullptr;           // supports of the current grid
    float radius = 0.f;
    bool auto_cell = false;                    // the current grid's cell was chosen per element (ws_nearest_neighbors, cell = 0)
    std::vector<int32_t> s_lens;               // per-element support counts of the current grid
    std::vector<int32_t> fills;                // caps of the fill launches of the last public entry (0: nb_nearest_kernel)
};

extern "C" {

int ws_neighbors_ws_create(ws_neighbors_ws** ws)
{
    WS_REQUIRE(ws, "NULL argument");
    *ws = new ws_neighbors_ws();
    return WS_OK;
}

void ws_neighbors_ws_destroy(ws_neighbors_ws* ws)
{
    if (!ws) return;
    ws->grids.release(); ws->bbox.release(); ws->cell_of.release(); ws->cell_start.release();
    ws->cursor.release(); ws->counts.release(); ws->scan_scratch.release(); ws->max_count.release();
    ws->sorted.release(); ws->sorted_alt.release(); ws->order.release();
    delete ws;
}

// bounding boxes, cell grids and the counting sort of the supports (no query work, no sync
// besides the staging copy of the per-element table)
static int nb_prepare(ws_neighbors_ws* ws, const float* queries, int64_t nq, const float* supports, int64_t ns,
                      const int32_t* h_q_lens, const int32_t* h_s_lens, int32_t nb, float radius, hipStream_t st,
                      bool auto_cell = false)      // auto_cell: nn_grid_setup_kernel picks the cell per element, `radius` is not read
{
    WS_REQUIRE(ws && h_q_lens && h_s_lens, "NULL argument");
    ws->fills.clear();
    WS_REQUIRE(nb >= 1 && nq >= 0 && ns >= 0, "bad sizes nb=%d nq=%lld ns=%lld", nb, (long long)nq, (long long)ns);
    WS_REQUIRE(ns < (1ll << 30) && nq < (1ll << 31), "point count exceeds int32 range");
    ws->max_count_host = 0;
    const bool reuse = ws->reuse_next;
    ws->reuse_next = false;
    if (reuse && ws->supports == supports && ws->ns == ns && ws->nb == nb && ws->radius == radius && ws->auto_cell == auto_cell &&
        nb <= GRID_TABLE_MAX && ws->max_count_word && nq > 0 && (int)ws->s_lens.size() == nb &&
        std::equal(ws->s_lens.begin(), ws->s_lens.end(), h_s_lens)) {
        // same supports, same radius as the previous plan (the caller vouches that the support DATA is unchanged):
        // bounding boxes, bins and the cell-sorted copy stay; only the query ranges and the counters are new
        QueryTable qt;
        int64_t qsum = 0;
        for (int b = 0; b < nb; ++b) {
            WS_REQUIRE(h_q_lens[b] >= 0, "negative batch length");
            qt.q_base[b] = (int)qsum; qt.q_len[b] = h_q_lens[b];
            qsum += h_q_lens[b];
        }
        WS_REQUIRE(qsum == nq, "batch lengths do not sum to the query count (%lld/%lld)", (long long)qsum, (long long)nq);
        WS_REQUIRE(queries, "NULL argument");
        int rc2;
        if ((rc2 = ws->counts.ensure((size_t)nq))) return rc2;
        nb_update_queries_kernel<<<1, 64, 0, st>>>(qt, nb, ws->grids.p);
        WS_LAUNCH_CHECK();
        WS_HIP(hipMemsetAsync(ws->max_count_word, 0, sizeof(int32_t), st));
        ws->self_query = (queries == supports && nq == ns);
        ws->queries = queries; ws->nq = nq;
        return WS_OK;
    }
    ws->nq = 0;
    std::vector<CloudGrid> hg((size_t)nb);
    int64_t qsum = 0, ssum = 0, cells = 0;
    for (int b = 0; b < nb; ++b) {
        WS_REQUIRE(h_q_lens[b] >= 0 && h_s_lens[b] >= 0, "negative batch length");
        CloudGrid& g = hg[(size_t)b];
        g = CloudGrid{};
        g.q_base = (int)qsum; g.q_len = h_q_lens[b];
        g.s_base = (int)ssum; g.s_len = h_s_lens[b];
        g.cell_base = (int)cells;
        g.cell_cap = 4 * h_s_lens[b] + 64;
        cells += g.cell_cap;
        qsum += h_q_lens[b]; ssum += h_s_lens[b];
    }
    WS_REQUIRE(qsum == nq && ssum == ns, "batch lengths do not sum to the point counts (%lld/%lld, %lld/%lld)",
               (long long)qsum, (long long)nq, (long long)ssum, (long long)ns);
    WS_REQUIRE(cells < (1ll << 31) - 2, "too many grid cells");
    if (nq == 0 || ns == 0) return ws_fail(WS_ERR_EMPTY, "Error");   // wrapper.cpp:201-205
    WS_REQUIRE(queries && supports, "NULL argument");

    int rc;
    if ((rc = ws->grids.ensure((size_t)nb))) return rc;
    if ((rc = ws->bbox.ensure((size_t)nb * 6))) return rc;
    if ((rc = ws->cell_of.ensure((size_t)ns))) return rc;
    if ((rc = ws->cell_start.ensure((size_t)cells + 2))) return rc;
    if ((rc = ws->cursor.ensure((size_t)cells + 2))) return rc;
    if ((rc = ws->counts.ensure((size_t)nq))) return rc;
    if ((rc = ws->scan_scratch.ensure((size_t)ws_scan_scratch_items(cells + 1)))) return rc;
    if ((rc = ws->max_count.ensure(1))) return rc;
    if ((rc = ws->sorted.ensure((size_t)ns))) return rc;
    if ((rc = ws->sorted_alt.ensure((size_t)ns))) return rc;
    if ((rc = ws->order.ensure((size_t)ns))) return rc;

    if (nb <= GRID_TABLE_MAX) {
        GridTable tbl;
        for (int b = 0; b < nb; ++b) tbl.g[b] = hg[(size_t)b];
        nb_upload_kernel<<<1, 64, 0, st>>>(tbl, nb, ws->grids.p);
        WS_LAUNCH_CHECK();
    } else {
        WS_HIP(hipMemcpyAsync(ws->grids.p, hg.data(), sizeof(CloudGrid) * (size_t)nb, hipMemcpyHostToDevice, st));
        WS_HIP(hipStreamSynchronize(st));   // hg is a stack-lifetime staging buffer
    }
    nb_bbox_kernel<<<nb, 1024, 0, st>>>(supports, ws->grids.p, ws->bbox.p);
    WS_LAUNCH_CHECK();
    if (auto_cell) nn_grid_setup_kernel<<<(nb + 63) / 64, 64, 0, st>>>(ws->grids.p, ws->bbox.p, nb);
    else nb_grid_setup_kernel<<<(nb + 63) / 64, 64, 0, st>>>(ws->grids.p, ws->bbox.p, nb, radius);
    WS_LAUNCH_CHECK();
    // one memset clears the cell histogram AND the max-count word (kept in the spare slot behind the scan output)
    WS_HIP(hipMemsetAsync(ws->cell_start.p, 0, sizeof(int32_t) * (size_t)(cells + 2), st));
    ws->max_count_word = ws->cell_start.p + cells + 1;
    nb_bin_count_kernel<<<ws_grid(ns, 256), 256, 0, st>>>(supports, ws->grids.p, nb, ns, ws->cell_of.p, ws->cell_start.p);
    WS_LAUNCH_CHECK();
    if ((rc = ws_exclusive_scan_i32(ws->cell_start.p, ws->cell_start.p, cells, ws->scan_scratch.p, st))) return rc;
    WS_HIP(hipMemcpyAsync(ws->cursor.p, ws->cell_start.p, sizeof(int32_t) * (size_t)(cells + 1), hipMemcpyDeviceToDevice, st));
    nb_bin_fill_kernel<<<ws_grid(ns, 256), 256, 0, st>>>(supports, ns, ws->cell_of.p, ws->cursor.p, ws->sorted_alt.p);
    WS_LAUNCH_CHECK();
    // entries of a cell in index order (the bin fill wrote them in arrival order): bit-identical grids from run to run
    nb_cell_rank_kernel<<<ws_grid(ns, 256), 256, 0, st>>>(ws->sorted_alt.p, ns, ws->cell_of.p, ws->cell_start.p, ws->sorted.p);
    WS_LAUNCH_CHECK();
    nb_order_kernel<<<ws_grid(ns, 256), 256, 0, st>>>(ws->sorted.p, ns, ws->order.p);
    WS_LAUNCH_CHECK();
    ws->self_query = (queries == supports && nq == ns);
    ws->queries = queries; ws->nq = nq; ws->ns = ns; ws->nb = nb; ws->cells = cells;
    ws->supports = supports; ws->radius = radius; ws->auto_cell = auto_cell;
    ws->s_lens.assign(h_s_lens, h_s_lens + nb);
    ws->r2 = radius * radius;   // neighbors.cpp:226
    return WS_OK;
}

// the opening of every entry that builds a plan: a prepare that fails leaves no plan behind
static int nb_begin(ws_neighbors_ws* ws, const float* queries, int64_t nq, const float* supports, int64_t ns,
                    const int32_t* h_q_lens, const int32_t* h_s_lens, int32_t nb, float radius, hipStream_t st,
                    bool auto_cell = false)
{
    const int rc = nb_prepare(ws, queries, nq, supports, ns, h_q_lens, h_s_lens, nb, radius, st, auto_cell);
    if (rc && ws) ws->nq = 0;
    return rc;
}

int ws_radius_neighbors_plan(ws_neighbors_ws* ws, const float* queries, int64_t nq, const float* supports,
                             int64_t ns, const int32_t* h_q_lens, const int32_t* h_s_lens, int32_t nb,
                             float radius, int32_t* h_max_count, void* stream)
{
    WS_REQUIRE(h_max_count, "NULL argument");
    *h_max_count = 0;
    hipStream_t st = (hipStream_t)stream;
    int rc = nb_begin(ws, queries, nq, supports, ns, h_q_lens, h_s_lens, nb, radius, st);
    if (rc) return rc;
    nb_count_kernel<<<ws_grid(nq, 4), 256, 0, st>>>(queries, nq, ws->grids.p, nb, ws->cell_start.p, ws->sorted.p, ws->r2,
                                                    ws->self_query ? ws->order.p : nullptr, ws->counts.p, ws->max_count_word);
    WS_LAUNCH_CHECK();
    int32_t mc = 0;
    WS_HIP(hipMemcpyAsync(&mc, ws->max_count_word, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    WS_HIP(hipStreamSynchronize(st));
    ws->max_count_host = mc;
    *h_max_count = mc;
    if (mc == 0) return ws_fail(WS_ERR_EMPTY, "Error");
    return WS_OK;
}

// the key_last request is one-shot: cleared when the public entry that consumed it returns
struct KeyLastGuard {
    ws_neighbors_ws* ws;
    ~KeyLastGuard() { if (ws) ws->key_last = nullptr; }
};

extern "C" int ws_nb_wide_caps = 1;       // 1: slab of the wide asynchronous search sized to the width (576 / 704 / 1024), 0: always 1024 (A/B: WEASAL_NB_WIDE_CAPS)
// grid cap of the fill launch on the ASYNCHRONOUS entries (the pyramid builders; the synchronous drop-in entries keep 4 096).  1 024 workgroups (4 per CU: the fill's queries are walked in cell order either way) instead of
// 4 096: alone the 13 searches of a pyramid take 1.29 instead of 1.08 ms, but they run under the training
// stream, which gets wave slots back -- DALES step 13.53 -> 13.42 ms, inference 5.20 -> 5.09 ms, config 5 38.7 -> 38.4 ms
constexpr int NB_MAX_BLOCKS = 1024;

// What one fill launch runs: the kernel, the slab it sorts rows of up to `cap` neighbours in, the output type and the grid cap.
// Built by nb_fill_plan alone; nb_launch_fill executes it and ws_radius_neighbors_fill_variant prints it.
enum NbFillKernel { NB_FILL_NONE, NB_FILL_NEAREST, NB_FILL_128, NB_FILL_WIDE, NB_FILL_2048 };
struct NbFillPlan {
    NbFillKernel kernel;      // NB_FILL_NONE: no slab holds `cap` neighbours
    int slab;                 // 128 (nb_fill128_kernel), 576 / 704 / 1024 (nb_fill_wide_kernel), 2048 (nb_fill_kernel); 0: nearest only
    bool out_i32;
    int max_blocks;           // grid cap
};

// cap == 0: the nearest-only search.  beside: the call comes through the asynchronous entries, i.e. from a pyramid builder working
// beside a training stream: the grid cap above applies; the synchronous entries (the drop-in `batch_query` and plan / fill) and
// the nearest-only search have the GPU to themselves: 4 096
static NbFillPlan nb_fill_plan(int cap, bool out_i32, bool beside)
{
    if (cap == 0) return {NB_FILL_NEAREST, 0, out_i32, 256 * 16};
    const int slab = cap <= 128 ? 128 : cap <= 576 ? 576 : cap <= 704 ? 704 : cap <= 1024 ? 1024 : cap <= 2048 ? 2048 : 0;
    const NbFillKernel kernel = !slab ? NB_FILL_NONE : slab == 128 ? NB_FILL_128 : slab == 2048 ? NB_FILL_2048 : NB_FILL_WIDE;
    return {kernel, slab, out_i32, beside ? NB_MAX_BLOCKS : 256 * 16};
}
static int nb_fill_unsupported(int cap)
{
    return ws_fail(WS_ERR_UNSUPPORTED, "max neighbour count %d exceeds the 2048-entry sort slab", cap);
}

// cap == 0 (nearest only): one index per query, `width` is not read and the word behind max_count_word becomes the any-hit flag
static int nb_launch_fill(ws_neighbors_ws* ws, int cap, int32_t width, int32_t* out_i32, int64_t* out_i64,
                          bool with_counts, hipStream_t st, bool beside = false)
{
    const NbFillPlan p = nb_fill_plan(cap, out_i32 != nullptr, beside);
    if (p.kernel == NB_FILL_NONE) return nb_fill_unsupported(cap);
    const int grid = ws_grid(ws->nq, 4, p.max_blocks);
    const int32_t* qo = ws->self_query ? ws->order.p : nullptr;
    int32_t* cn = with_counts ? ws->counts.p : nullptr;
    int32_t* mx = with_counts ? ws->max_count_word : nullptr;
    unsigned long long* kl = ws->key_last;
    const bool called = dispatch([&](auto i32, auto sl) {
        using OT = std::conditional_t<i32.value != 0, int32_t, int64_t>;
        OT* out = i32.value ? (OT*)out_i32 : (OT*)out_i64;
        if constexpr (sl.value == 0)
            nb_nearest_kernel<OT><<<grid, 256, 0, st>>>(ws->queries, ws->nq, ws->grids.p, ws->nb, ws->cell_start.p, ws->sorted.p, ws->r2, ws->ns,
                                                        qo, out, ws->max_count_word);
        else if constexpr (sl.value == 128)
            nb_fill128_kernel<OT><<<grid, 256, 0, st>>>(ws->queries, ws->nq, ws->grids.p, ws->nb, ws->cell_start.p, ws->sorted.p, ws->r2, ws->ns,
                                                        width, qo, out, cn, mx, kl);
        else if constexpr (sl.value == 2048)
            nb_fill_kernel<2048, OT><<<grid, 256, 0, st>>>(ws->queries, ws->nq, ws->grids.p, ws->nb, ws->cell_start.p, ws->sorted.p, ws->r2, ws->ns,
                                                           width, qo, out, cn, mx, kl);
        else
            nb_fill_wide_kernel<OT, sl.value><<<grid, 256, 0, st>>>(ws->queries, ws->nq, ws->grids.p, ws->nb, ws->cell_start.p, ws->sorted.p, ws->r2,
                                                                    ws->ns, width, qo, out, cn, mx, kl);
    }, Flag{p.out_i32}, Pick<0, 128, 576, 704, 1024, 2048>{p.slab});
    if (!called) return ws_no_instantiation("neighbour fill: slab=%d (cap=%d)", p.slab, cap);
    WS_LAUNCH_CHECK();
    ws->fills.push_back(cap);
    return WS_OK;
}

int ws_radius_neighbors_fill_variant(int32_t cap, int32_t out_i32, int32_t beside, char* out, int32_t out_cap)
{
    WS_REQUIRE(out && out_cap > 0 && cap >= 0, "bad argument");
    const NbFillPlan p = nb_fill_plan(cap, out_i32 != 0, beside != 0);
    const char* t = p.out_i32 ? "int32" : "int64";
    switch (p.kernel) {
    case NB_FILL_NONE: return nb_fill_unsupported(cap);
    case NB_FILL_NEAREST: snprintf(out, (size_t)out_cap, "nb_nearest_kernel<%s> grid<=%d", t, p.max_blocks); break;
    case NB_FILL_128: snprintf(out, (size_t)out_cap, "nb_fill128_kernel<%s> grid<=%d", t, p.max_blocks); break;
    case NB_FILL_2048: snprintf(out, (size_t)out_cap, "nb_fill_kernel<2048,%s> grid<=%d", t, p.max_blocks); break;
    case NB_FILL_WIDE: snprintf(out, (size_t)out_cap, "nb_fill_wide_kernel<%s,%d> grid<=%d", t, p.slab, p.max_blocks); break;
    }
    return WS_OK;
}

int ws_radius_neighbors_last_fills(const ws_neighbors_ws* ws, int32_t* caps, int32_t max, int32_t* n)
{
    WS_REQUIRE(ws && n && max >= 0 && (caps || max == 0), "NULL argument");
    *n = (int32_t)ws->fills.size();
    for (int32_t i = 0; i < *n && i < max; ++i) caps[i] = ws->fills[(size_t)i];
    return WS_OK;
}

int ws_radius_neighbors_search(ws_neighbors_ws* ws, const float* queries, int64_t nq, const float* supports,
                               int64_t ns, const int32_t* h_q_lens, const int32_t* h_s_lens, int32_t nb,
                               float radius, int32_t width, int32_t* out_i32, int64_t* out_i64,
                               int32_t* h_max_count, void* stream)
{
    KeyLastGuard guard{ws};
    WS_REQUIRE(h_max_count, "NULL argument");
    WS_REQUIRE((out_i32 != nullptr) != (out_i64 != nullptr), "exactly one of out_i32 / out_i64 must be given");
    WS_REQUIRE(width >= 1, "width must be >= 1");
    *h_max_count = 0;
    hipStream_t st = (hipStream_t)stream;
    int rc = nb_begin(ws, queries, nq, supports, ns, h_q_lens, h_s_lens, nb, radius, st);
    if (rc) return rc;
    int cap = width > 128 ? 1024 : 128;      // wide rows are asked for: the bucketed sort from the start
    for (;;) {
        WS_HIP(hipMemsetAsync(ws->max_count_word, 0, sizeof(int32_t), st));
        if ((rc = nb_launch_fill(ws, cap, width, out_i32, out_i64, true, st))) return rc;
        int32_t mc = 0;
        WS_HIP(hipMemcpyAsync(&mc, ws->max_count_word, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        WS_HIP(hipStreamSynchronize(st));
        ws->max_count_host = mc;
        *h_max_count = mc;
        if (mc == 0) return ws_fail(WS_ERR_EMPTY, "Error");
        if (mc <= cap) return WS_OK;
        cap = mc;      // a row overflowed the sort slab: run once more with a slab that fits
    }
}

// Row slab of the asynchronous search for rows of `width` entries.  The slab must hold EVERY neighbour inside the radius (the row
// keeps the nearest `width` of them); the calibrated limits are 90th percentiles of the counts, the largest count of a batch lies
// 5-20 % above them (config 5: limits 422 / 519 / 472, maxima 491 / 552 / 565), so 5/4 of the width rounded up to the next
// kernel variant covers it with fewer LDS bytes per wave (4 instead of 3 workgroups per CU); a batch that does overflow is
// reported through d_max_count and redone by the caller, as before.
int32_t ws_radius_neighbors_async_cap(int32_t width)
{
    if (width <= 128) return 128;
    if (!ws_nb_wide_caps) return 1024;
    const int need = width + width / 4;
    return need <= 576 ? 576 : (need <= 704 ? 704 : 1024);
}

int ws_radius_neighbors_search_async(ws_neighbors_ws* ws, const float* queries, int64_t nq, const float* supports,
                                     int64_t ns, const int32_t* h_q_lens, const int32_t* h_s_lens, int32_t nb,
                                     float radius, int32_t width, int32_t* out_i32, int64_t* out_i64,
                                     int32_t* d_max_count, void* stream)
{
    KeyLastGuard guard{ws};
    WS_REQUIRE(d_max_count, "NULL argument");
    WS_REQUIRE((out_i32 != nullptr) != (out_i64 != nullptr), "exactly one of out_i32 / out_i64 must be given");
    WS_REQUIRE(width >= 1, "width must be >= 1");
    hipStream_t st = (hipStream_t)stream;
    int rc = nb_begin(ws, queries, nq, supports, ns, h_q_lens, h_s_lens, nb, radius, st);
    if (rc) return rc;
    // rows wider than the 128-entry fast path are asked for (deformable radius): the 1024-key bucketed sort from the start,
    // instead of a 128-entry pass the caller would have to repeat
    const int cap = ws_radius_neighbors_async_cap(width);
    if ((rc = nb_launch_fill(ws, cap, width, out_i32, out_i64, true, st, true))) return rc;   // max-count word cleared by nb_prepare
    WS_HIP(hipMemcpyAsync(d_max_count, ws->max_count_word, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    ws->max_count_host = cap;   // unknown on the host; rows beyond the slab are reported through d_max_count
    return WS_OK;
}

int ws_radius_neighbors_histogram(ws_neighbors_ws* ws, const float* queries, int64_t nq, const float* supports,
                                  int64_t ns, const int32_t* h_q_lens, const int32_t* h_s_lens, int32_t nb,
                                  float radius, int64_t* hist, int32_t hist_n, void* stream)
{
    KeyLastGuard guard{ws};
    WS_REQUIRE(hist, "NULL argument");
    WS_REQUIRE(hist_n >= 1, "hist_n must be >= 1");
    if (hist_n > WS_NB_HIST_MAX)
        return ws_fail(WS_ERR_UNSUPPORTED, "hist_n = %d exceeds the %d bins a workgroup keeps in LDS", hist_n, WS_NB_HIST_MAX);
    hipStream_t st = (hipStream_t)stream;
    int rc = nb_begin(ws, queries, nq, supports, ns, h_q_lens, h_s_lens, nb, radius, st);
    if (rc) return rc;
    // at least 16 queries per workgroup (4 per wave) behind every flush; the grid cap of the asynchronous entries
    const int grid = ws_grid(nq, 16, NB_MAX_BLOCKS);
    nb_hist_kernel<<<grid, 256, sizeof(int) * (size_t)hist_n, st>>>(queries, nq, ws->grids.p, nb, ws->cell_start.p, ws->sorted.p, ws->r2,
                                                                     ws->self_query ? ws->order.p : nullptr,
                                                                     reinterpret_cast<unsigned long long*>(hist), hist_n);
    WS_LAUNCH_CHECK();
    return WS_OK;       // no row lengths on the host: ws->max_count_host stays 0, a fill needs a plan of its own
}

int ws_radius_neighbors_nearest_async(ws_neighbors_ws* ws, const float* queries, int64_t nq, const float* supports,
                                      int64_t ns, const int32_t* h_q_lens, const int32_t* h_s_lens, int32_t nb,
                                      float radius, int32_t* out_i32, int64_t* out_i64, int32_t* d_any, void* stream)
{
    KeyLastGuard guard{ws};
    WS_REQUIRE(d_any, "NULL argument");
    WS_REQUIRE((out_i32 != nullptr) != (out_i64 != nullptr), "exactly one of out_i32 / out_i64 must be given");
    hipStream_t st = (hipStream_t)stream;
    int rc = nb_begin(ws, queries, nq, supports, ns, h_q_lens, h_s_lens, nb, radius, st);
    if (rc) return rc;
    if ((rc = nb_launch_fill(ws, 0, 1, out_i32, out_i64, false, st))) return rc;
    WS_HIP(hipMemcpyAsync(d_any, ws->max_count_word, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    ws->max_count_host = 1;
    return WS_OK;
}

int ws_radius_neighbors_fill(ws_neighbors_ws* ws, int32_t width, int32_t* out_i32, int64_t* out_i64, void* stream)
{
    KeyLastGuard guard{ws};
    WS_REQUIRE(ws && ws->nq > 0 && ws->max_count_host > 0, "no successful plan to fill from");
    WS_REQUIRE((out_i32 != nullptr) != (out_i64 != nullptr), "exactly one of out_i32 / out_i64 must be given");
    WS_REQUIRE(width >= 1 && width <= ws->max_count_host, "width %d outside [1, max_count=%d]", width, ws->max_count_host);
    ws->fills.clear();
    return nb_launch_fill(ws, ws->max_count_host, width, out_i32, out_i64, false, (hipStream_t)stream);
}

int ws_radius_neighbors_order(const ws_neighbors_ws* ws, int32_t* out_order, void* stream)
{
    WS_REQUIRE(ws && ws->ns > 0 && out_order, "no plan / NULL argument");
    WS_HIP(hipMemcpyAsync(out_order, ws->order.p, sizeof(int32_t) * (size_t)ws->ns, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return WS_OK;
}

const int32_t* ws_radius_neighbors_counts(const ws_neighbors_ws* ws) { return ws ? ws->counts.p : nullptr; }

int ws_radius_neighbors_reuse_grid(ws_neighbors_ws* ws, int32_t on)
{
    WS_REQUIRE(ws, "NULL argument");
    ws->reuse_next = on != 0;
    return WS_OK;
}

int ws_radius_neighbors_set_key_last(ws_neighbors_ws* ws, uint64_t* d_key_last)
{
    WS_REQUIRE(ws, "NULL argument");
    ws->key_last = reinterpret_cast<unsigned long long*>(d_key_last);
    return WS_OK;
}

int ws_radius_neighbors_grid_info(const ws_neighbors_ws* ws, int32_t* nb, int64_t* cells, int64_t* ns, int64_t* blob_bytes)
{
    WS_REQUIRE(ws && ws->nq > 0 && nb && cells && ns && blob_bytes, "no plan / NULL argument");
    *nb = ws->nb; *cells = ws->cells; *ns = ws->ns;
    *blob_bytes = ws_grid_blob_bytes(ws->nb, ws->cells, ws->ns);
    return WS_OK;
}

int ws_radius_neighbors_grid_export(const ws_neighbors_ws* ws, void* blob, void* stream)
{
    WS_REQUIRE(ws && ws->nq > 0 && blob, "no plan / NULL argument");
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)blob;
    WS_HIP(hipMemcpyAsync(base, ws->grids.p, sizeof(CloudGrid) * (size_t)ws->nb, hipMemcpyDeviceToDevice, st));
    WS_HIP(hipMemcpyAsync(base + ws_grid_blob_cells_off(ws->nb), ws->cell_start.p, sizeof(int32_t) * (size_t)(ws->cells + 2),
                          hipMemcpyDeviceToDevice, st));
    WS_HIP(hipMemcpyAsync(base + ws_grid_blob_sorted_off(ws->nb, ws->cells), ws->sorted.p, sizeof(float4) * (size_t)ws->ns,
                          hipMemcpyDeviceToDevice, st));
    return WS_OK;
}

// Exact nearest support of every query (nearest_kernels.h).  The grid is K1's: nb_prepare with radius = cell builds it for any
// cell size (its cap loop may enlarge the cell: the walk reads the grid's own inv_cell), cell = 0 lets nn_grid_setup_kernel
// choose.  The edge contract differs from the radius entries', so the arguments are checked here first: nb_prepare then
// only ever sees nq > 0 and ns > 0.
int ws_nearest_neighbors(ws_neighbors_ws* ws, const float* queries, int64_t nq, const float* supports, int64_t ns,
                         const int32_t* h_q_lens, const int32_t* h_s_lens, int32_t nb, float cell, int32_t* out_i32,
                         int64_t* out_i64, double* out_d2, int32_t* d_status, void* stream)
{
    KeyLastGuard guard{ws};
    WS_REQUIRE(ws && h_q_lens && h_s_lens, "NULL argument");
    WS_REQUIRE((out_i32 != nullptr) != (out_i64 != nullptr), "exactly one of out_i32 / out_i64 must be given");
    WS_REQUIRE(nb >= 1 && nq >= 0 && ns >= 0, "bad sizes nb=%d nq=%lld ns=%lld", nb, (long long)nq, (long long)ns);
    WS_REQUIRE(ns < (1ll << 30) && nq < (1ll << 31), "point count exceeds int32 range");
    WS_REQUIRE(cell >= 0.f && cell < 3.0e38f, "cell must be finite and >= 0 (0: chosen by the library)");
    int64_t qsum = 0, ssum = 0;
    for (int b = 0; b < nb; ++b) {
        WS_REQUIRE(h_q_lens[b] >= 0 && h_s_lens[b] >= 0, "negative batch length");
        qsum += h_q_lens[b]; ssum += h_s_lens[b];
    }
    WS_REQUIRE(qsum == nq && ssum == ns, "batch lengths do not sum to the point counts (%lld/%lld, %lld/%lld)",
               (long long)qsum, (long long)nq, (long long)ssum, (long long)ns);
    WS_REQUIRE(nq == 0 || queries, "NULL argument");
    WS_REQUIRE(nq == 0 || ns == 0 || supports, "NULL argument");
    if (nq == 0) return WS_OK;
    hipStream_t st = (hipStream_t)stream;
    ws->reuse_next = false;       // a grid of this entry is never taken from a radius plan
    if (ns > 0) {
        const int rc = nb_begin(ws, queries, nq, supports, ns, h_q_lens, h_s_lens, nb, cell, st, cell == 0.f);
        if (rc) return rc;
    }
    const int grid = ws_grid(nq, 256);
    dispatch([&](auto i32) {
        using OT = std::conditional_t<i32.value != 0, int32_t, int64_t>;
        OT* out = i32.value ? (OT*)out_i32 : (OT*)out_i64;
        if (ns == 0)
            nn_none_kernel<OT><<<grid, 256, 0, st>>>(nq, ns, out, out_d2);
        else
            nn_exact_kernel<OT><<<grid, 256, 0, st>>>(queries, nq, ws->grids.p, nb, ws->cell_start.p, ws->sorted.p, ns,
                                                      ws->self_query ? ws->order.p : nullptr, out, out_d2, d_status);
    }, Flag{out_i32 != nullptr});
    WS_LAUNCH_CHECK();
    // no counts, no rows, and a cell that may differ per element: nothing a fill, an export or a reused grid could continue from
    ws->nq = 0;
    ws->fills.clear();
    ws->supports = nullptr;
    return WS_OK;
}

}  // extern "C"
