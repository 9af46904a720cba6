// weasal_amd/csrc/anchors.hip -- the weak-label anchors of a tile (utils/anchors.py), from points resident in HBM.
//
//   ws_anchor_bounds          :33-38    the six min / max of the cloud.
//   ws_anchor_members_plan    :83-99    per anchor, the number of points inside its sphere and the classes among them
//   ws_anchor_members_fill    :91-103   the survivors (n > 0) in their order, each with its ascending point list
//   ws_anchor_pairs_plan/fill :114-121  neighbouring anchors (i < j, centres within 1.5 * sub_radius)
//   ws_anchor_overlap_plan    :126-134  per pair, the size of the intersection when the label rows differ
//   ws_anchor_overlap_fill    :130-138  the new anchors: intersection, AND of the rows, mean of the members
//
// Arithmetic (compiled with -ffp-contract=off): a float32 coordinate widened to float64, d = p - a per axis,
// d2 = (dx*dx + dy*dy) + dz*dz with every product and sum rounded, member iff d2 <= radius*radius.  Everything else is
// integers, so the results do not depend on the order the atomics arrive in: counts are integer sums, label bits an OR,
// and the lists, filled through atomic cursors, are sorted per anchor afterwards.
//
// The search structure is a uniform grid over the ANCHORS (the small side), built by the caller: cell >= radius, so that
// the members of an anchor lie in the 27 cells around the point's own.  The grid only proposes candidates; the comparison
// above decides.  Index lists from the caller (sel) are range-checked: an entry outside is skipped and counted in status.
#include "ws_scan.h"

namespace {

typedef unsigned long long u64;

constexpr int AN_BLOCK = 256;
constexpr int AN_SORT_LDS = 8192;         // longest list the per-anchor sort keeps in LDS (int32 keys: 32 KiB)

struct Grid {
    double ox, oy, oz, cell;
    int nx, ny, nz;
};

__device__ __forceinline__ void status_add(int64_t* status, int which)
{
    atomicAdd((u64*)status + which, 1ull);
}

__device__ __forceinline__ double dist2(double px, double py, double pz, const double* __restrict__ a)
{
    const double dx = px - a[0], dy = py - a[1], dz = pz - a[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// cell coordinate of v along one axis, clamped to [-2, n + 1] (a NaN goes to -2: nothing is near it)
__device__ __forceinline__ int cell_of(double v, double o, double cell, int n)
{
    const double f = floor((v - o) / cell);
    if (!(f >= -2.0)) return -2;
    if (f > (double)(n + 1)) return n + 1;
    return (int)f;
}

// ---- bounds ----------------------------------------------------------------------------------------------------------
// order-preserving map float -> uint32, so that integer atomicMin / atomicMax order the floats
__device__ __forceinline__ unsigned f2key(float f)
{
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float key2f(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? k & 0x7FFFFFFFu : ~k);
}

__global__ void bounds_init_kernel(unsigned* __restrict__ keys)
{
    if (threadIdx.x < 6) keys[threadIdx.x] = (threadIdx.x & 1) ? 0u : 0xFFFFFFFFu;      // min slots, max slots
}

__global__ __launch_bounds__(AN_BLOCK) void bounds_kernel(const float* __restrict__ pts, int64_t n, unsigned* __restrict__ keys)
{
    __shared__ unsigned lds[6];
    if (threadIdx.x < 6) lds[threadIdx.x] = (threadIdx.x & 1) ? 0u : 0xFFFFFFFFu;
    __syncthreads();
    unsigned lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    for (int64_t i = (int64_t)blockIdx.x * AN_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * AN_BLOCK) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const unsigned k = f2key(pts[i * 3 + d]);
            lo[d] = k < lo[d] ? k : lo[d];
            hi[d] = k > hi[d] ? k : hi[d];
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned a = __shfl_xor(lo[d], o, 64), b = __shfl_xor(hi[d], o, 64);
            lo[d] = a < lo[d] ? a : lo[d];
            hi[d] = b > hi[d] ? b : hi[d];
        }
        if (ws_lane() == 0) {
            atomicMin(&lds[2 * d], lo[d]);
            atomicMax(&lds[2 * d + 1], hi[d]);
        }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        if (threadIdx.x & 1) atomicMax(&keys[threadIdx.x], lds[threadIdx.x]);
        else atomicMin(&keys[threadIdx.x], lds[threadIdx.x]);
    }
}

__global__ void bounds_decode_kernel(unsigned* __restrict__ keys)
{
    if (threadIdx.x < 6) keys[threadIdx.x] = __float_as_uint(key2f(keys[threadIdx.x]));
}

// ---- members ---------------------------------------------------------------------------------------------------------
// One point per lane, 27 cells of the anchor grid.  FILL = false: counts[a] += 1 and bits[a] |= 1 << label;
// FILL = true: idx[ptr32[a] + cursor[a]++] = i (the order inside a list is fixed by members_sort_kernel).
template <bool FILL>
__global__ __launch_bounds__(AN_BLOCK) void members_kernel(const float* __restrict__ pts, const int32_t* __restrict__ labels,
                                                           int64_t n, int n_class, const double* __restrict__ anchors, Grid g,
                                                           double r2, const int32_t* __restrict__ cell_start,
                                                           const int32_t* __restrict__ cell_item, int32_t* __restrict__ counts,
                                                           uint32_t* __restrict__ bits, const int32_t* __restrict__ slot,
                                                           const int32_t* __restrict__ ptr32, int64_t* __restrict__ idx,
                                                           int64_t* __restrict__ status)
{
    for (int64_t i = (int64_t)blockIdx.x * AN_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * AN_BLOCK) {
        const double px = (double)pts[i * 3], py = (double)pts[i * 3 + 1], pz = (double)pts[i * 3 + 2];
        uint32_t bit = 0u;
        if (!FILL) {
            const int32_t lb = labels[i];
            if (lb >= 0 && lb < n_class) bit = 1u << lb;
            else status_add(status, WS_ANCHOR_BAD_LABEL);
        }
        const int cx = cell_of(px, g.ox, g.cell, g.nx), cy = cell_of(py, g.oy, g.cell, g.ny), cz = cell_of(pz, g.oz, g.cell, g.nz);
        for (int x = cx - 1; x <= cx + 1; ++x) {
            if (x < 0 || x >= g.nx) continue;
            for (int y = cy - 1; y <= cy + 1; ++y) {
                if (y < 0 || y >= g.ny) continue;
                const int z0 = cz - 1 < 0 ? 0 : cz - 1, z1 = cz + 1 >= g.nz ? g.nz - 1 : cz + 1;
                if (z0 > z1) continue;
                const int64_t row = ((int64_t)x * g.ny + y) * g.nz;            // z is the fastest axis: one contiguous run
                const int beg = cell_start[row + z0], end = cell_start[row + z1 + 1];
                for (int e = beg; e < end; ++e) {
                    const int a = cell_item[e];
                    if (!(dist2(px, py, pz, anchors + (int64_t)a * 3) <= r2)) continue;
                    if (!FILL) {
                        atomicAdd(&counts[a], 1);                               // results unused: the return-less forms
                        if (bit && !(bits[a] & bit)) atomicOr(&bits[a], bit);   // (a stale read only repeats the OR)
                    } else {
                        const int pos = atomicAdd(&counts[a], 1);               // counts: the cursors, zeroed by the caller
                        idx[(int64_t)ptr32[a] + pos] = i;
                    }
                }
            }
        }
    }
}

// flags[a] = counts[a] > 0 and the 64-bit sum of the counts (the int32 scan would wrap silently past 2^31)
__global__ __launch_bounds__(AN_BLOCK) void flags_total_kernel(const int32_t* __restrict__ counts, int64_t n, int32_t* __restrict__ flags,
                                                               int64_t* __restrict__ total)
{
    u64 s = 0;
    for (int64_t i = (int64_t)blockIdx.x * AN_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * AN_BLOCK) {
        const int32_t c = counts[i];
        if (flags) flags[i] = c > 0;
        s += (u64)(c > 0 ? c : 0);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (ws_lane() == 0 && s) atomicAdd((u64*)total, s);
}

// totals[w] = (int64) last[0]: the grand total an exclusive scan leaves in its slot n
__global__ void copy_total_kernel(const int32_t* __restrict__ last, int64_t* __restrict__ dst)
{
    if (threadIdx.x == 0) *dst = (int64_t)*last;
}

__global__ __launch_bounds__(AN_BLOCK) void members_rows_kernel(const double* __restrict__ anchors, int64_t a0,
                                                                const int32_t* __restrict__ counts, const int32_t* __restrict__ slot,
                                                                const int32_t* __restrict__ ptr32, const uint32_t* __restrict__ bits,
                                                                int64_t* __restrict__ kept, int64_t* __restrict__ out_ptr,
                                                                double* __restrict__ centres, uint32_t* __restrict__ out_bits)
{
    for (int64_t a = (int64_t)blockIdx.x * AN_BLOCK + threadIdx.x; a <= a0; a += (int64_t)gridDim.x * AN_BLOCK) {
        if (a == a0) { out_ptr[slot[a0]] = (int64_t)ptr32[a0]; continue; }
        if (counts[a] <= 0) continue;
        const int s = slot[a];
        kept[s] = a;
        out_ptr[s] = (int64_t)ptr32[a];
        out_bits[s] = bits[a];
        centres[(int64_t)s * 3] = anchors[a * 3];
        centres[(int64_t)s * 3 + 1] = anchors[a * 3 + 1];
        centres[(int64_t)s * 3 + 2] = anchors[a * 3 + 2];
    }
}

// One workgroup per list: ascending sort by the bitonic network in its all-ascending form (the first stage of a merge
// compares i with its mirror in the block, the others i with i ^ j), so that the slots past the end, which read as
// +infinity, are never moved and any length works.  Lists up to AN_SORT_LDS entries are sorted in LDS as int32 (point ids
// are < 2^31, checked by the host), longer ones where they lie.
__global__ __launch_bounds__(AN_BLOCK) void members_sort_kernel(const int64_t* __restrict__ row_ptr, int64_t rows, int64_t* __restrict__ idx)
{
    extern __shared__ int32_t keys[];
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {             // (uniform trip count for the workgroup)
        const int64_t beg = row_ptr[r];
        const int64_t len = row_ptr[r + 1] - beg;
        if (len < 2) continue;
        int64_t* v = idx + beg;
        int64_t p2 = 2;
        while (p2 < len) p2 <<= 1;
        const bool in_lds = len <= AN_SORT_LDS;
        if (in_lds) {
            for (int64_t t = threadIdx.x; t < len; t += AN_BLOCK) keys[t] = (int32_t)v[t];
        }
        __syncthreads();
        for (int64_t k = 2; k <= p2; k <<= 1) {
            for (int64_t j = k >> 1; j > 0; j >>= 1) {
                const bool first = j == (k >> 1);
                for (int64_t t = threadIdx.x; t < (p2 >> 1); t += AN_BLOCK) {
                    const int64_t off = t % j;
                    const int64_t lo = (t / j) * (j << 1) + off;                         // the lower index of the t-th pair
                    const int64_t hi = first ? lo + k - 1 - 2 * off : lo + j;
                    if (hi >= len) continue;
                    if (in_lds) {
                        const int32_t a = keys[lo], b = keys[hi];
                        if (a > b) { keys[lo] = b; keys[hi] = a; }
                    } else {
                        const int64_t a = v[lo], b = v[hi];
                        if (a > b) { v[lo] = b; v[hi] = a; }
                    }
                }
                __syncthreads();
            }
        }
        if (in_lds) {
            for (int64_t t = threadIdx.x; t < len; t += AN_BLOCK) v[t] = (int64_t)keys[t];
        }
        __syncthreads();
    }
}

// ---- neighbouring anchors --------------------------------------------------------------------------------------------
// One position s of the selection per lane; its partners are the positions t > s whose centre is within the threshold.
// The grid lists POSITIONS.  FILL: the partners are written at pair_ptr[s], then insertion-sorted (a row holds a handful).
template <bool FILL>
__global__ __launch_bounds__(AN_BLOCK) void pairs_kernel(const double* __restrict__ centres, int64_t na, const int64_t* __restrict__ sel,
                                                         int64_t ns, Grid g, double r2, const int32_t* __restrict__ cell_start,
                                                         const int32_t* __restrict__ cell_item, int32_t* __restrict__ pair_cnt,
                                                         const int32_t* __restrict__ pair_ptr, int32_t* __restrict__ pair_i,
                                                         int32_t* __restrict__ pair_j, int64_t* __restrict__ status)
{
    for (int64_t s = (int64_t)blockIdx.x * AN_BLOCK + threadIdx.x; s < ns; s += (int64_t)gridDim.x * AN_BLOCK) {
        const int64_t a = sel ? sel[s] : s;
        if (a < 0 || a >= na) {
            if (!FILL) { pair_cnt[s] = 0; status_add(status, WS_ANCHOR_BAD_SEL); }
            continue;
        }
        const double px = centres[a * 3], py = centres[a * 3 + 1], pz = centres[a * 3 + 2];
        const int cx = cell_of(px, g.ox, g.cell, g.nx), cy = cell_of(py, g.oy, g.cell, g.ny), cz = cell_of(pz, g.oz, g.cell, g.nz);
        int cnt = 0;
        const int base = FILL ? pair_ptr[s] : 0;
        for (int x = cx - 1; x <= cx + 1; ++x) {
            if (x < 0 || x >= g.nx) continue;
            for (int y = cy - 1; y <= cy + 1; ++y) {
                if (y < 0 || y >= g.ny) continue;
                const int z0 = cz - 1 < 0 ? 0 : cz - 1, z1 = cz + 1 >= g.nz ? g.nz - 1 : cz + 1;
                if (z0 > z1) continue;
                const int64_t row = ((int64_t)x * g.ny + y) * g.nz;
                const int beg = cell_start[row + z0], end = cell_start[row + z1 + 1];
                for (int e = beg; e < end; ++e) {
                    const int t = cell_item[e];
                    if (t <= s) continue;
                    const int64_t b = sel ? sel[t] : t;
                    if (b < 0 || b >= na) continue;
                    if (!(dist2(px, py, pz, centres + b * 3) <= r2)) continue;
                    if (FILL) {
                        int q = cnt;                                                      // insertion: ascending t
                        while (q > 0 && pair_j[base + q - 1] > t) { pair_j[base + q] = pair_j[base + q - 1]; --q; }
                        pair_j[base + q] = t;
                        pair_i[base + cnt] = (int32_t)s;
                    }
                    ++cnt;
                }
            }
        }
        if (!FILL) pair_cnt[s] = cnt;
    }
}

// ---- overlaps --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool contains(const int64_t* __restrict__ v, int64_t n, int64_t key)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (v[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && v[lo] == key;
}

// the two lists of pair p, the shorter first (the intersection comes out ascending either way); false: no new anchor
__device__ __forceinline__ bool pair_lists(int64_t p, const int32_t* __restrict__ pair_i, const int32_t* __restrict__ pair_j,
                                           const int64_t* __restrict__ sel, const int64_t* __restrict__ ptr,
                                           const int64_t* __restrict__ idx, int64_t nnz, const uint32_t* __restrict__ bits,
                                           const int64_t*& la, int64_t& na, const int64_t*& lb, int64_t& nb, uint32_t& both)
{
    const int64_t a = sel ? sel[pair_i[p]] : pair_i[p], b = sel ? sel[pair_j[p]] : pair_j[p];     // in range: pairs_kernel
    const uint32_t ba = bits[a], bb = bits[b];
    if (ba == bb) return false;
    both = ba & bb;
    int64_t a0 = ptr[a], a1 = ptr[a + 1], b0 = ptr[b], b1 = ptr[b + 1];
    if (a0 < 0 || a1 > nnz || b0 < 0 || b1 > nnz || a1 <= a0 || b1 <= b0) return false;
    la = idx + a0; na = a1 - a0; lb = idx + b0; nb = b1 - b0;
    if (na > nb) {
        const int64_t* tl = la; la = lb; lb = tl;
        const int64_t tn = na; na = nb; nb = tn;
    }
    return true;
}

// one wave per pair: every member of the shorter list is looked up in the longer one
__global__ __launch_bounds__(AN_BLOCK) void overlap_count_kernel(const int64_t* __restrict__ ptr, const int64_t* __restrict__ idx,
                                                                 int64_t nnz, const uint32_t* __restrict__ bits,
                                                                 const int64_t* __restrict__ sel, const int32_t* __restrict__ pair_i,
                                                                 const int32_t* __restrict__ pair_j, int64_t n_pairs,
                                                                 int32_t* __restrict__ inter_cnt)
{
    const int lane = ws_lane();
    for (int64_t p = (int64_t)blockIdx.x * (AN_BLOCK / 64) + (threadIdx.x >> 6); p < n_pairs; p += (int64_t)gridDim.x * (AN_BLOCK / 64)) {
        const int64_t *la, *lb;
        int64_t na, nb;
        uint32_t both;
        int cnt = 0;
        if (pair_lists(p, pair_i, pair_j, sel, ptr, idx, nnz, bits, la, na, lb, nb, both)) {
            for (int64_t base = 0; base < na; base += 64) {
                const int64_t k = base + lane;
                const bool hit = k < na && contains(lb, nb, la[k]);
                cnt += __popcll(__ballot(hit));
            }
        }
        if (lane == 0) inter_cnt[p] = cnt;
    }
}

__global__ __launch_bounds__(AN_BLOCK) void sel_len_kernel(const int64_t* __restrict__ ptr, int64_t nnz, int64_t na,
                                                           const int64_t* __restrict__ sel, int64_t ns, int32_t* __restrict__ len)
{
    for (int64_t s = (int64_t)blockIdx.x * AN_BLOCK + threadIdx.x; s < ns; s += (int64_t)gridDim.x * AN_BLOCK) {
        const int64_t a = sel ? sel[s] : s;
        int64_t l = 0;
        if (a >= 0 && a < na) {
            const int64_t b = ptr[a], e = ptr[a + 1];
            if (b >= 0 && e <= nnz && e > b) l = e - b;
        }
        len[s] = (int32_t)l;
    }
}

// one wave per output row: rows [0, ns) copy the selected anchors, rows ns + new_slot[p] are the new anchors of the pairs
__global__ __launch_bounds__(AN_BLOCK) void overlap_fill_kernel(const float* __restrict__ pts, int64_t n, const int64_t* __restrict__ ptr,
                                                                const int64_t* __restrict__ idx, int64_t nnz,
                                                                const uint32_t* __restrict__ bits, const double* __restrict__ centres,
                                                                int64_t na, const int64_t* __restrict__ sel, int64_t ns,
                                                                const int32_t* __restrict__ pair_i, const int32_t* __restrict__ pair_j,
                                                                int64_t n_pairs, const int32_t* __restrict__ inter_cnt,
                                                                const int32_t* __restrict__ new_slot, const int32_t* __restrict__ new_ptr,
                                                                const int32_t* __restrict__ sel_ptr, int64_t n_new, int64_t nnz_new,
                                                                int64_t nnz_sel, int64_t* __restrict__ out_ptr,
                                                                int64_t* __restrict__ out_idx, uint32_t* __restrict__ out_bits,
                                                                double* __restrict__ out_centres)
{
    const int lane = ws_lane();
    const int64_t items = ns + n_pairs;
    for (int64_t it = (int64_t)blockIdx.x * (AN_BLOCK / 64) + (threadIdx.x >> 6); it < items; it += (int64_t)gridDim.x * (AN_BLOCK / 64)) {
        if (it < ns) {
            const int64_t a = sel ? sel[it] : it;
            const int64_t o = sel_ptr[it], len = sel_ptr[it + 1] - o;
            const bool ok = a >= 0 && a < na;
            if (lane == 0) {
                out_ptr[it] = o;
                out_bits[it] = ok ? bits[a] : 0u;
            }
            if (lane < 3) out_centres[it * 3 + lane] = ok ? centres[a * 3 + lane] : 0.0;
            if (ok)
                for (int64_t k = lane; k < len; k += 64) out_idx[o + k] = idx[ptr[a] + k];
            if (it == 0 && lane == 0) out_ptr[ns + n_new] = nnz_sel + nnz_new;
            continue;
        }
        const int64_t p = it - ns;
        if (inter_cnt[p] <= 0) continue;
        const int64_t *la, *lb;
        int64_t la_n, lb_n;
        uint32_t both;
        if (!pair_lists(p, pair_i, pair_j, sel, ptr, idx, nnz, bits, la, la_n, lb, lb_n, both)) continue;
        const int64_t row = ns + new_slot[p], o = nnz_sel + new_ptr[p];
        double sx = 0.0, sy = 0.0, sz = 0.0;
        int64_t run = 0;
        for (int64_t base = 0; base < la_n; base += 64) {
            const int64_t k = base + lane;
            int64_t v = -1;
            bool hit = false;
            if (k < la_n) { v = la[k]; hit = contains(lb, lb_n, v); }
            const u64 m = __ballot(hit);
            if (hit) {
                out_idx[o + run + __popcll(m & ((1ull << lane) - 1ull))] = v;
                if (v >= 0 && v < n) { sx += (double)pts[v * 3]; sy += (double)pts[v * 3 + 1]; sz += (double)pts[v * 3 + 2]; }
            }
            run += __popcll(m);
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {                                   // a fixed tree: the same sum on every run
            sx += __shfl_xor(sx, s, 64); sy += __shfl_xor(sy, s, 64); sz += __shfl_xor(sz, s, 64);
        }
        if (lane == 0) {
            out_ptr[row] = o;
            out_bits[row] = both;
            const double cnt = (double)run;
            out_centres[row * 3] = sx / cnt;
            out_centres[row * 3 + 1] = sy / cnt;
            out_centres[row * 3 + 2] = sz / cnt;
        }
    }
}

int read_grid(const double* h_grid, Grid& g)
{
    WS_REQUIRE(h_grid, "NULL grid");
    g.ox = h_grid[0]; g.oy = h_grid[1]; g.oz = h_grid[2]; g.cell = h_grid[3];
    g.nx = (int)h_grid[4]; g.ny = (int)h_grid[5]; g.nz = (int)h_grid[6];
    WS_REQUIRE(g.cell > 0.0 && g.nx >= 1 && g.ny >= 1 && g.nz >= 1 && (int64_t)g.nx * g.ny * g.nz <= (1ll << 26),
               "bad grid: cell=%g dims=%d x %d x %d", g.cell, g.nx, g.ny, g.nz);
    return WS_OK;
}

}  // namespace

extern "C" {

int ws_anchor_bounds(const float* points, int64_t n, float* bounds, void* stream)
{
    WS_REQUIRE(n >= 1 && points && bounds, "ws_anchor_bounds: needs at least one point (n=%lld)", (long long)n);
    hipStream_t st = (hipStream_t)stream;
    bounds_init_kernel<<<1, 64, 0, st>>>((unsigned*)bounds);
    WS_LAUNCH_CHECK();
    bounds_kernel<<<ws_grid(n, AN_BLOCK * 8, 1024), AN_BLOCK, 0, st>>>(points, n, (unsigned*)bounds);
    WS_LAUNCH_CHECK();
    bounds_decode_kernel<<<1, 64, 0, st>>>((unsigned*)bounds);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int64_t ws_anchor_scratch_bytes(int64_t items)
{
    return (int64_t)sizeof(int32_t) * (ws_scan_scratch_items(items < 0 ? 0 : items) + (items < 0 ? 0 : items) + 1);
}

int ws_anchor_members_plan(const float* points, const int32_t* labels, int64_t n, int32_t n_class, const double* anchors, int64_t a0,
                           double radius, const double* h_grid, const int32_t* cell_start, const int32_t* cell_item,
                           int32_t* counts, int32_t* slot, int32_t* ptr32, uint32_t* bits, int64_t* totals, int64_t* status,
                           void* scratch, void* stream)
{
    WS_REQUIRE(n >= 0 && a0 >= 1 && radius >= 0.0, "bad sizes n=%lld anchors=%lld radius=%g", (long long)n, (long long)a0, radius);
    if (n_class < 1 || n_class > 32) return ws_fail(WS_ERR_UNSUPPORTED, "ws_anchor_members_plan: n_class=%d (1 to 32)", n_class);
    if (n >= (1ll << 31) || a0 >= (1ll << 31))
        return ws_fail(WS_ERR_UNSUPPORTED, "ws_anchor_members_plan: n=%lld, anchors=%lld (below 2^31)", (long long)n, (long long)a0);
    WS_REQUIRE((n == 0 || (points && labels)) && anchors && cell_start && cell_item && counts && slot && ptr32 && bits && totals &&
               status && scratch, "NULL argument");
    Grid g;
    int rc = read_grid(h_grid, g);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    WS_HIP(hipMemsetAsync(counts, 0, sizeof(int32_t) * (a0 + 1), st));
    WS_HIP(hipMemsetAsync(bits, 0, sizeof(uint32_t) * a0, st));
    WS_HIP(hipMemsetAsync(totals, 0, sizeof(int64_t) * WS_ANCHOR_TOTAL_WORDS, st));
    if (n > 0) {
        members_kernel<false><<<ws_grid(n, AN_BLOCK, 1 << 16), AN_BLOCK, 0, st>>>(points, labels, n, n_class, anchors, g, radius * radius,
                                                                                 cell_start, cell_item, counts, bits, nullptr, nullptr,
                                                                                 nullptr, status);
        WS_LAUNCH_CHECK();
    }
    int32_t* flags = (int32_t*)scratch;
    int32_t* scan_scratch = flags + a0 + 1;
    flags_total_kernel<<<ws_grid(a0, AN_BLOCK * 4, 1024), AN_BLOCK, 0, st>>>(counts, a0, flags, totals + WS_ANCHOR_TOTAL_NNZ);
    WS_LAUNCH_CHECK();
    rc = ws_exclusive_scan_i32(flags, slot, a0, scan_scratch, st);
    if (rc) return rc;
    rc = ws_exclusive_scan_i32(counts, ptr32, a0, scan_scratch, st);
    if (rc) return rc;
    copy_total_kernel<<<1, 64, 0, st>>>(slot + a0, totals + WS_ANCHOR_TOTAL_ROWS);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_anchor_members_fill(const float* points, int64_t n, const double* anchors, int64_t a0, double radius, const double* h_grid,
                           const int32_t* cell_start, const int32_t* cell_item, int32_t* counts, const int32_t* slot,
                           const int32_t* ptr32, const uint32_t* bits, int64_t n_kept, int64_t nnz, int64_t* kept, int64_t* anchor_ptr,
                           int64_t* anchor_idx, double* centres, uint32_t* anchor_bits, int32_t* cursor, void* stream)
{
    WS_REQUIRE(n >= 0 && a0 >= 1 && n_kept >= 0 && n_kept <= a0 && nnz >= 0, "bad sizes n=%lld anchors=%lld kept=%lld nnz=%lld",
               (long long)n, (long long)a0, (long long)n_kept, (long long)nnz);
    if (nnz >= (1ll << 31))
        return ws_fail(WS_ERR_CAPACITY, "ws_anchor_members_fill: %lld members in all (the lists are planned with 32-bit offsets)",
                       (long long)nnz);
    if (n >= (1ll << 31)) return ws_fail(WS_ERR_UNSUPPORTED, "ws_anchor_members_fill: n=%lld (below 2^31)", (long long)n);
    WS_REQUIRE(anchors && cell_start && cell_item && counts && slot && ptr32 && bits && anchor_ptr && cursor &&
               (n_kept == 0 || (kept && centres && anchor_bits)) && (nnz == 0 || (anchor_idx && points)), "NULL argument");
    Grid g;
    int rc = read_grid(h_grid, g);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    members_rows_kernel<<<ws_grid(a0 + 1, AN_BLOCK, 4096), AN_BLOCK, 0, st>>>(anchors, a0, counts, slot, ptr32, bits, kept, anchor_ptr,
                                                                            centres, anchor_bits);
    WS_LAUNCH_CHECK();
    if (nnz == 0) return WS_OK;
    WS_HIP(hipMemsetAsync(cursor, 0, sizeof(int32_t) * a0, st));
    members_kernel<true><<<ws_grid(n, AN_BLOCK, 1 << 16), AN_BLOCK, 0, st>>>(points, nullptr, n, 0, anchors, g, radius * radius, cell_start,
                                                                            cell_item, cursor, nullptr, slot, ptr32, anchor_idx, nullptr);
    WS_LAUNCH_CHECK();
    members_sort_kernel<<<ws_grid(n_kept, 1, 1 << 16), AN_BLOCK, sizeof(int32_t) * AN_SORT_LDS, st>>>(anchor_ptr, n_kept, anchor_idx);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_anchor_pairs_plan(const double* centres, int64_t n_anchors, const int64_t* sel, int64_t n_sel, double radius,
                         const double* h_grid, const int32_t* cell_start, const int32_t* cell_item, int32_t* pair_cnt,
                         int32_t* pair_ptr, int64_t* totals, int64_t* status, void* scratch, void* stream)
{
    WS_REQUIRE(n_anchors >= 1 && n_sel >= 1 && radius >= 0.0, "bad sizes anchors=%lld sel=%lld radius=%g", (long long)n_anchors,
               (long long)n_sel, radius);
    if (n_anchors >= (1ll << 31) || n_sel >= (1ll << 31))
        return ws_fail(WS_ERR_UNSUPPORTED, "ws_anchor_pairs_plan: anchors=%lld sel=%lld (below 2^31)", (long long)n_anchors, (long long)n_sel);
    WS_REQUIRE(centres && cell_start && cell_item && pair_cnt && pair_ptr && totals && status && scratch, "NULL argument");
    Grid g;
    int rc = read_grid(h_grid, g);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    WS_HIP(hipMemsetAsync(totals, 0, sizeof(int64_t) * WS_ANCHOR_TOTAL_WORDS, st));
    pairs_kernel<false><<<ws_grid(n_sel, AN_BLOCK, 4096), AN_BLOCK, 0, st>>>(centres, n_anchors, sel, n_sel, g, radius * radius, cell_start,
                                                                            cell_item, pair_cnt, nullptr, nullptr, nullptr, status);
    WS_LAUNCH_CHECK();
    flags_total_kernel<<<ws_grid(n_sel, AN_BLOCK * 4, 1024), AN_BLOCK, 0, st>>>(pair_cnt, n_sel, nullptr, totals + WS_ANCHOR_TOTAL_ROWS);
    WS_LAUNCH_CHECK();
    return ws_exclusive_scan_i32(pair_cnt, pair_ptr, n_sel, (int32_t*)scratch, st);
}

int ws_anchor_pairs_fill(const double* centres, int64_t n_anchors, const int64_t* sel, int64_t n_sel, double radius,
                         const double* h_grid, const int32_t* cell_start, const int32_t* cell_item, const int32_t* pair_ptr,
                         int64_t n_pairs, int32_t* pair_i, int32_t* pair_j, void* stream)
{
    WS_REQUIRE(n_anchors >= 1 && n_sel >= 1 && n_pairs >= 0, "bad sizes anchors=%lld sel=%lld pairs=%lld", (long long)n_anchors,
               (long long)n_sel, (long long)n_pairs);
    if (n_pairs >= (1ll << 31)) return ws_fail(WS_ERR_CAPACITY, "ws_anchor_pairs_fill: %lld pairs (below 2^31)", (long long)n_pairs);
    if (n_pairs == 0) return WS_OK;
    WS_REQUIRE(centres && cell_start && cell_item && pair_ptr && pair_i && pair_j, "NULL argument");
    Grid g;
    int rc = read_grid(h_grid, g);
    if (rc) return rc;
    pairs_kernel<true><<<ws_grid(n_sel, AN_BLOCK, 4096), AN_BLOCK, 0, (hipStream_t)stream>>>(centres, n_anchors, sel, n_sel, g,
                                                                                            radius * radius, cell_start, cell_item, nullptr,
                                                                                            pair_ptr, pair_i, pair_j, nullptr);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_anchor_overlap_plan(const int64_t* anchor_ptr, const int64_t* anchor_idx, int64_t nnz, const uint32_t* anchor_bits,
                           int64_t n_anchors, const int64_t* sel, int64_t n_sel, const int32_t* pair_i, const int32_t* pair_j,
                           int64_t n_pairs, int32_t* inter_cnt, int32_t* new_slot, int32_t* new_ptr, int32_t* sel_ptr, int64_t* totals,
                           void* scratch, void* stream)
{
    WS_REQUIRE(n_anchors >= 1 && n_sel >= 1 && n_pairs >= 0 && nnz >= 0, "bad sizes anchors=%lld sel=%lld pairs=%lld nnz=%lld",
               (long long)n_anchors, (long long)n_sel, (long long)n_pairs, (long long)nnz);
    if (n_pairs >= (1ll << 31) || n_sel >= (1ll << 31))
        return ws_fail(WS_ERR_UNSUPPORTED, "ws_anchor_overlap_plan: pairs=%lld sel=%lld (below 2^31)", (long long)n_pairs, (long long)n_sel);
    WS_REQUIRE(anchor_ptr && anchor_bits && (nnz == 0 || anchor_idx) && inter_cnt && new_slot && new_ptr && sel_ptr && totals && scratch &&
               (n_pairs == 0 || (pair_i && pair_j)), "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const int64_t items = n_pairs > n_sel ? n_pairs : n_sel;
    int32_t* tmp = (int32_t*)scratch;                     // [items + 1]: flags of the pairs, then the lengths of the selection
    int32_t* scan_scratch = tmp + items + 1;
    WS_HIP(hipMemsetAsync(totals, 0, sizeof(int64_t) * WS_ANCHOR_TOTAL_WORDS, st));
    if (n_pairs > 0) {
        overlap_count_kernel<<<ws_grid(n_pairs, AN_BLOCK / 64, 1 << 16), AN_BLOCK, 0, st>>>(anchor_ptr, anchor_idx, nnz, anchor_bits, sel,
                                                                                           pair_i, pair_j, n_pairs, inter_cnt);
        WS_LAUNCH_CHECK();
        flags_total_kernel<<<ws_grid(n_pairs, AN_BLOCK * 4, 1024), AN_BLOCK, 0, st>>>(inter_cnt, n_pairs, tmp, totals + WS_ANCHOR_TOTAL_NNZ);
        WS_LAUNCH_CHECK();
    }
    int rc = ws_exclusive_scan_i32(tmp, new_slot, n_pairs, scan_scratch, st);
    if (rc) return rc;
    rc = ws_exclusive_scan_i32(inter_cnt, new_ptr, n_pairs, scan_scratch, st);
    if (rc) return rc;
    copy_total_kernel<<<1, 64, 0, st>>>(new_slot + n_pairs, totals + WS_ANCHOR_TOTAL_ROWS);
    WS_LAUNCH_CHECK();
    sel_len_kernel<<<ws_grid(n_sel, AN_BLOCK, 4096), AN_BLOCK, 0, st>>>(anchor_ptr, nnz, n_anchors, sel, n_sel, tmp);
    WS_LAUNCH_CHECK();
    flags_total_kernel<<<ws_grid(n_sel, AN_BLOCK * 4, 1024), AN_BLOCK, 0, st>>>(tmp, n_sel, nullptr, totals + WS_ANCHOR_TOTAL_BASE);
    WS_LAUNCH_CHECK();
    return ws_exclusive_scan_i32(tmp, sel_ptr, n_sel, scan_scratch, st);
}

int ws_anchor_overlap_fill(const float* points, int64_t n, const int64_t* anchor_ptr, const int64_t* anchor_idx, int64_t nnz,
                           const uint32_t* anchor_bits, const double* centres, int64_t n_anchors, const int64_t* sel, int64_t n_sel,
                           const int32_t* pair_i, const int32_t* pair_j, int64_t n_pairs, const int32_t* inter_cnt,
                           const int32_t* new_slot, const int32_t* new_ptr, const int32_t* sel_ptr, int64_t n_new, int64_t nnz_new,
                           int64_t nnz_sel, int64_t* out_ptr, int64_t* out_idx, uint32_t* out_bits, double* out_centres, void* stream)
{
    WS_REQUIRE(n >= 0 && n_anchors >= 1 && n_sel >= 1 && n_pairs >= 0 && n_new >= 0 && n_new <= n_pairs && nnz_new >= 0 && nnz_sel >= 0,
               "bad sizes n=%lld anchors=%lld sel=%lld pairs=%lld new=%lld", (long long)n, (long long)n_anchors, (long long)n_sel,
               (long long)n_pairs, (long long)n_new);
    if (nnz_new >= (1ll << 31) || nnz_sel >= (1ll << 31))
        return ws_fail(WS_ERR_CAPACITY, "ws_anchor_overlap_fill: %lld + %lld members (the lists are planned with 32-bit offsets)",
                       (long long)nnz_sel, (long long)nnz_new);
    WS_REQUIRE(anchor_ptr && anchor_bits && centres && inter_cnt && new_slot && new_ptr && sel_ptr && out_ptr && out_bits && out_centres &&
               (nnz == 0 || anchor_idx) && (nnz_sel + nnz_new == 0 || out_idx) && (nnz_new == 0 || points) &&
               (n_pairs == 0 || (pair_i && pair_j)), "NULL argument");
    overlap_fill_kernel<<<ws_grid(n_sel + n_pairs, AN_BLOCK / 64, 1 << 16), AN_BLOCK, 0, (hipStream_t)stream>>>(
        points, n, anchor_ptr, anchor_idx, nnz, anchor_bits, centres, n_anchors, sel, n_sel, pair_i, pair_j, n_pairs, inter_cnt, new_slot,
        new_ptr, sel_ptr, n_new, nnz_new, nnz_sel, out_ptr, out_idx, out_bits, out_centres);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

}  // extern "C"
