// weasal_amd/csrc/sampler.hip -- the sphere sampler of the potential-based datasets, on tiles resident in HBM
// (datasets/DALES_PseudoLabel.py:265-518 `potential_item` with datasets/common.py:252-334 `augmentation_transform`).
//
// The reference cuts one sphere at a time on the host: arg-min of the potentials, two KD-tree radius queries, numpy, and
// loops until the batch holds more than batch_limit points.  Which sphere comes next depends on the potentials the last
// one left, and whether there is a next one depends on the running point count: both live on the device here, so the
// host queues the chain for `max_spheres` spheres at once and reads one small state block back when it is through.
//
// Three launches per sphere, every one of the same shape whatever the data (the grid is sized by the largest tile):
//   sphere_scan_kernel    workgroups [0, gp): pick (cloud, point, centre), the Tukey-updated potentials of their chunk
//                         computed but NOT stored, partial (min, first arg-min) of them; workgroups [gp, gp + gn): pick,
//                         count the members of the sphere in their chunk of the cloud's points
//   sphere_decide_kernel  one workgroup: final arg-min, exclusive scan of the gn counts, then the decisions of
//                         DALES_PseudoLabel.py:364-408 -- dropped (n < 2), does not fit the output buffer (overflow: the
//                         sphere is left undone, potentials untouched, so a second call with a larger buffer resumes with
//                         exactly this sphere), or kept (row offset, batch full?)
//   sphere_emit_kernel    workgroups [0, gp): store the updated potentials (same expression, same bits as the scan);
//                         workgroups [gp, gp + gn): members of their chunk in ASCENDING index order at the sphere's row
//                         offset -- centred points, augmentation, features, labels, input indices
// Two additions leave that chain as it is (ws_sampler_batch_items):
//   colours   a cloud may carry sub_colors [n, ncol] (ws_sampler_set_colors; Vaihingen3D_PseudoLabel.py:366, :379-383): the
//             emit body copies them in front of the two height columns, or writes +0 for a slot whose colour_keep is 0;
//   random    centres from a list (cloud, point) on the device instead of the potentials (`random_item`, DALES_PseudoLabel.py
//             :520-640): gp = 0, so no workgroup touches a potential; `pick` reads epoch_inds[*epoch_i] and the decide kernel
//             advances epoch_i with every sphere it commits (kept or dropped), never with one it leaves undone.
// The class-balanced draw of those centres (`*Sampler.__iter__`, :941-992) is a select-by-rank on the resident labels:
//   class_count_kernel    per (cloud, chunk): members of every class in the chunk
//   class_scan_kernel     per cloud: exclusive scan of every class's chunk counts, totals [n_clouds, n_class] (the host reads
//                         these, draws POSITIONS with its own stream and uploads (cloud, class, position) triples)
//   class_select_kernel   per triple: chunk by binary search in the scanned counts, then the rank inside that one chunk
// Every kernel starts by reading `done` and returns when it is set.  Membership is tested twice (count, emit) instead of
// being stored: 12 bytes read per point against 4 written and 4 read for a flag array, and no N-sized scratch.
//
// Arithmetic: float64 for centre, distances and potentials, float32 for the augmentation, every operation rounded on its
// own (this file is compiled with -ffp-contract=off and spells the operations out), in the order the reference's numpy
// and sklearn code evaluates them.
#include "ws_common.h"
#include "ws_argmin.h"
#include "ws_scan.h"
#include <vector>

#define WS_SAMPLER_MAX_SPHERES 64       /* = WS_PYRAMID_MAX_BATCH */
#define WS_SAMPLER_MAX_CLOUDS 4096
#define WS_SAMPLER_GP 256               /* workgroups over the potential points, at most */
#define WS_SAMPLER_GN 1024              /* workgroups over the cloud's points, at most (4 counts per thread in the decide kernel) */
#define WS_SAMPLER_MAX_CLASSES 64       /* classes of the centre draw */
#define WS_SAMPLER_MAX_COLORS 3

namespace {

struct WsCloud {
    const float* pts;        // [n,3]
    const int32_t* labels;   // [n] or NULL
    const float* pot_pts;    // [p,3]
    double* pot;             // [p]
    long long n, p;
    const float* colors;     // [n,ncol] or NULL
    long long ncol;
};

struct WsDraw {              // host-drawn values of one sphere slot (72 bytes, mirrored by weasal_amd/sampler.py)
    double noise[3];
    float rot[9];
    float scale[3];
};

struct WsSlot {
    long long n, cloud, point, row, ord;
    double c[3];
};

struct WsState {             // ws_sampler_state_bytes(): 8 + 64 * 8 int64 / float64 words
    long long done, overflow, n_spheres, n_fail, row_off, attempts, cur_slot, cur_flags;
    WsSlot slots[WS_SAMPLER_MAX_SPHERES];
};

struct WsArgs {
    const WsCloud* clouds;
    int nc;
    double* min_pot;
    long long* argmin;
    const WsDraw* draws;
    WsState* st;
    double* pv;
    long long* pi;
    int* counts;
    int gp, gn;
    double r2;
    int max_slots;
    long long batch_limit, capacity;
    float aug_noise;
    unsigned long long seed, seq0;
    int fd;
    const int32_t* lut;
    int lut_n, labels_zero, update_pot;
    float* out_points;
    float* out_features;
    long long* out_labels;
    long long* out_inds;
    int32_t* out_lengths;
    float* out_scales;
    float* out_rots;
    int32_t* out_cloud_inds;
    int32_t* out_point_inds;
    const int32_t* keep;               // colour_keep per slot, or NULL (every slot keeps its colours)
    int ncol;
    int random;                        // centres from epoch_inds
    const long long* epoch_inds;       // [2, n_centres]
    long long n_centres;
    long long* epoch_i;
};

// reduced distance of the tree: ((dx^2 + dy^2) + dz^2) in float64, d = f64(point) - centre
__device__ __forceinline__ double rdist(const float* __restrict__ p, long long i, const double* c)
{
    const double dx = __dsub_rn((double)p[3 * i], c[0]), dy = __dsub_rn((double)p[3 * i + 1], c[1]),
                 dz = __dsub_rn((double)p[3 * i + 2], c[2]);
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

// potential of coarse point i after the Tukey update (DALES_PseudoLabel.py:340-347): dists = sqrt(rd), d2 = dists^2,
// tukey = (1 - d2 / r^2)^2, zero where d2 > r^2
__device__ __forceinline__ double tukey_new(const float* __restrict__ p, double v, long long i, const double* c, double r2, bool& hit)
{
    const double rd = rdist(p, i, c);
    hit = rd <= r2;
    if (!hit) return v;
    const double dist = __dsqrt_rn(rd);
    const double d2 = __dmul_rn(dist, dist);
    const double t = __dsub_rn(1.0, __ddiv_rn(d2, r2));
    return __dadd_rn(v, d2 > r2 ? 0.0 : __dmul_rn(t, t));
}

// :322-333 -- cloud = first arg-min of the per-cloud minima, point = its arg-min, centre = f64(pot_points[point]) + noise.
// Called by all 256 threads; sv / si are free again on return.
__device__ __forceinline__ void pick(const WsArgs& a, int k, double* sv, long long* si, int& cloud, long long& point, double* c)
{
    if (a.random) {          // DALES_PseudoLabel.py:534-535, :547-551: centre = f64(sub_points[point]) + noise
        long long e = *a.epoch_i;
        e = e < 0 ? 0 : (e >= a.n_centres ? a.n_centres - 1 : e);
        long long cl = a.epoch_inds[e], pt = a.epoch_inds[a.n_centres + e];
        cl = cl < 0 ? 0 : (cl >= a.nc ? a.nc - 1 : cl);            // a list from outside stays inside the tables
        const long long n = a.clouds[cl].n;
        pt = pt < 0 ? 0 : (pt >= n ? n - 1 : pt);
        cloud = (int)cl;
        point = pt;
        const float* pp = a.clouds[cl].pts;
#pragma unroll
        for (int j = 0; j < 3; ++j) c[j] = __dadd_rn((double)pp[3 * pt + j], a.draws[k].noise[j]);
        return;
    }
    double best = 1.0e308;
    long long bi = -1;
    for (int e = threadIdx.x; e < a.nc; e += 256) ws_argmin_take(best, bi, a.min_pot[e], e);
    ws_argmin_block(best, bi, sv, si);
    cloud = si[0] < 0 ? 0 : (int)si[0];
    __syncthreads();
    point = a.argmin[cloud];
    const float* pp = a.clouds[cloud].pot_pts;
#pragma unroll
    for (int j = 0; j < 3; ++j) c[j] = __dadd_rn((double)pp[3 * point + j], a.draws[k].noise[j]);
}

__device__ __forceinline__ void chunk(long long n, int nblk, int b, long long& beg, long long& end)
{
    const long long per = (n + nblk - 1) / nblk;
    beg = (long long)b * per;
    if (beg > n) beg = n;
    end = beg + per < n ? beg + per : n;
}

__global__ __launch_bounds__(256) void sampler_init_kernel(WsState* st, int resume)
{
    if (resume) {
        if (threadIdx.x == 0) { st->done = 0; st->overflow = 0; st->cur_flags = 0; }
        return;
    }
    long long* w = (long long*)st;
    for (int e = threadIdx.x; e < (int)(sizeof(WsState) / 8); e += 256) w[e] = 0;
}

__global__ __launch_bounds__(256) void sphere_scan_kernel(WsArgs a)
{
    __shared__ double sv[256];
    __shared__ long long si[256];
    __shared__ int lds[WS_SCAN_BLOCK / 64 + 1];
    if (a.st->done) return;
    const int k = (int)a.st->attempts;
    if (k >= a.max_slots) return;
    int cloud;
    long long point;
    double c[3];
    pick(a, k, sv, si, cloud, point, c);
    const WsCloud cl = a.clouds[cloud];
    if ((int)blockIdx.x < a.gp) {
        long long beg, end;
        chunk(cl.p, a.gp, blockIdx.x, beg, end);
        double best = 1.0e308;
        long long bi = -1;
        for (long long i = beg + threadIdx.x; i < end; i += 256) {
            bool hit;
            const double v = a.update_pot ? tukey_new(cl.pot_pts, cl.pot[i], i, c, a.r2, hit) : cl.pot[i];
            ws_argmin_take(best, bi, v, i);
        }
        ws_argmin_block(best, bi, sv, si);
        if (threadIdx.x == 0) { a.pv[blockIdx.x] = sv[0]; a.pi[blockIdx.x] = si[0]; }
    } else {
        const int b = blockIdx.x - a.gp;
        long long beg, end;
        chunk(cl.n, a.gn, b, beg, end);
        int cnt = 0;
        for (long long i = beg + threadIdx.x; i < end; i += 256) cnt += rdist(cl.pts, i, c) <= a.r2 ? 1 : 0;
        int total;
        ws_block_exclusive_scan(cnt, lds, total);
        if (threadIdx.x == 0) a.counts[b] = total;
    }
}

__global__ __launch_bounds__(256) void sphere_decide_kernel(WsArgs a)
{
    __shared__ double sv[256];
    __shared__ long long si[256];
    __shared__ int lds[WS_SCAN_BLOCK / 64 + 1];
    WsState* st = a.st;
    const long long was_done = st->done;
    const int k = (int)st->attempts;
    __syncthreads();
    if (was_done || k >= a.max_slots) {
        if (threadIdx.x == 0) { st->cur_flags = 0; st->done = 1; }
        return;
    }
    int cloud;
    long long point;
    double c[3];
    pick(a, k, sv, si, cloud, point, c);
    double best = 1.0e308;
    long long bi = -1;
    for (int e = threadIdx.x; e < a.gp; e += 256) ws_argmin_take(best, bi, a.pv[e], a.pi[e]);
    ws_argmin_block(best, bi, sv, si);
    const double new_min = sv[0];
    const long long new_arg = si[0];
    // counts[b] -> exclusive offsets, in place (gn <= 4 * 256)
    int v[4], s = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int j = threadIdx.x * 4 + e;
        v[e] = j < a.gn ? a.counts[j] : 0;
        s += v[e];
    }
    int total;
    int run = ws_block_exclusive_scan(s, lds, total);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int j = threadIdx.x * 4 + e;
        if (j < a.gn) a.counts[j] = run;
        run += v[e];
    }
    if (threadIdx.x != 0) return;
    WsSlot& sl = st->slots[k];
    sl.cloud = cloud;
    sl.point = point;
    sl.c[0] = c[0]; sl.c[1] = c[1]; sl.c[2] = c[2];
    sl.n = total;
    sl.ord = -1;
    sl.row = st->row_off;
    st->cur_slot = k;
    long long flags = 0;
    if (total < 2) {                                       // :367-373 the sphere is dropped, its potentials stay updated
        st->n_fail += 1;
        st->attempts = k + 1;
        flags = 1;
    } else if (st->row_off + total > a.capacity) {         // left undone: nothing of it is written, nothing committed
        st->overflow = 1;
        st->done = 1;
    } else {
        sl.ord = st->n_spheres;
        st->n_spheres += 1;
        st->row_off += total;
        st->attempts = k + 1;
        flags = 3;
        if (st->row_off > a.batch_limit) st->done = 1;     // :404-408
    }
    if ((flags & 1) && a.update_pot && new_arg >= 0) {
        a.min_pot[cloud] = new_min;
        a.argmin[cloud] = new_arg;
    }
    if ((flags & 1) && a.random) {                         // :538-540, once per attempted sphere
        const long long e = *a.epoch_i + 1;
        *a.epoch_i = e >= a.n_centres ? e - a.n_centres : e;
    }
    if (st->attempts >= a.max_slots) st->done = 1;
    st->cur_flags = flags;
}

// N(0,1) as a pure function of (seed, sphere sequence number, row of the sphere, column): the counter hash of
// ws_dropout_apply (splitmix64 finaliser) keyed per sphere, two 24-bit uniforms, Box-Muller
__device__ __forceinline__ float sampler_normal(unsigned long long key, unsigned long long row, int j)
{
    const unsigned long long ctr = (row * 3ull + (unsigned long long)j) * 2ull;
    const unsigned h0 = ws_drop_hash(key, ctr), h1 = ws_drop_hash(key, ctr + 1ull);
    const float u1 = (float)((h0 >> 8) + 1u) * 5.9604644775390625e-8f;      // (0, 1]
    const float u2 = (float)(h1 >> 8) * 5.9604644775390625e-8f;             // [0, 1)
    return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

__global__ __launch_bounds__(256) void sphere_emit_kernel(WsArgs a)
{
    __shared__ int lds[WS_SCAN_BLOCK / 64 + 1];
    const WsState* st = a.st;
    const long long flags = st->cur_flags;
    if (flags == 0) return;
    const int k = (int)st->cur_slot;
    const WsSlot sl = st->slots[k];
    const WsCloud cl = a.clouds[sl.cloud];
    const double c[3] = {sl.c[0], sl.c[1], sl.c[2]};
    if ((int)blockIdx.x < a.gp) {
        if (!a.update_pot) return;
        long long beg, end;
        chunk(cl.p, a.gp, blockIdx.x, beg, end);
        for (long long i = beg + threadIdx.x; i < end; i += 256) {
            bool hit;
            const double v = tukey_new(cl.pot_pts, cl.pot[i], i, c, a.r2, hit);
            if (hit) cl.pot[i] = v;
        }
        return;
    }
    if (!(flags & 2)) return;
    const int b = blockIdx.x - a.gp;
    const WsDraw dr = a.draws[k];
    const bool keep_col = !a.keep || a.keep[k] != 0;
    if (b == 0 && threadIdx.x == 0) {                      // the per-sphere tail of the input list (:419-427, :456)
        const long long o = sl.ord;
        a.out_lengths[o] = (int32_t)sl.n;
        a.out_cloud_inds[o] = (int32_t)sl.cloud;
        a.out_point_inds[o] = (int32_t)sl.point;
        for (int e = 0; e < 3; ++e) a.out_scales[3 * o + e] = dr.scale[e];
        for (int e = 0; e < 9; ++e) a.out_rots[9 * o + e] = dr.rot[e];
    }
    long long beg, end;
    chunk(cl.n, a.gn, b, beg, end);
    long long local = a.counts[b];                         // row inside the sphere of this chunk's first member
    unsigned long long key = a.seed + (a.seq0 + (unsigned long long)k) * 0xD1B54A32D192ED03ull;
    key = (key ^ (key >> 31)) * 0x9E3779B97F4A7C15ull;
    for (long long t0 = beg; t0 < end; t0 += 256) {
        const long long i = t0 + threadIdx.x;
        const int f = (i < end && rdist(cl.pts, i, c) <= a.r2) ? 1 : 0;
        int tot;
        const int pos = ws_block_exclusive_scan(f, lds, tot);
        if (f) {
            const long long in_sphere = local + pos, row = sl.row + in_sphere;
            float p[3], q[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) p[j] = (float)__dsub_rn((double)cl.pts[3 * i + j], c[j]);        // :376
#pragma unroll
            for (int j = 0; j < 3; ++j) {                                                                 // common.py:316
                float v = __fadd_rn(__fadd_rn(__fmul_rn(p[0], dr.rot[j]), __fmul_rn(p[1], dr.rot[3 + j])), __fmul_rn(p[2], dr.rot[6 + j]));
                v = __fmul_rn(v, dr.scale[j]);
                if (a.aug_noise != 0.0f) v = __fadd_rn(v, __fmul_rn(a.aug_noise, sampler_normal(key, (unsigned long long)in_sphere, j)));
                q[j] = v;
                a.out_points[3 * row + j] = v;
            }
            float* fr = a.out_features + row * a.fd;
            fr[0] = 1.0f;
            // [colours..., f32(f64(z') + centre_z), z'] cut to fd - 1 columns (:389, :430-434; Vaihingen3D_PseudoLabel.py
            // :379-383, :424-432)
            for (int e = 0; e < a.fd - 1; ++e) {
                float v;
                if (e < a.ncol) v = keep_col ? cl.colors[i * a.ncol + e] : 0.0f;
                else if (e == a.ncol) v = (float)__dadd_rn((double)q[2], c[2]);
                else v = q[2];
                fr[1 + e] = v;
            }
            long long lab = 0;
            if (!a.labels_zero) {                                                                         // :377-381
                lab = cl.labels[i];
                if (a.lut) lab = (lab >= 0 && lab < a.lut_n) ? a.lut[lab] : -1;
            }
            a.out_labels[row] = lab;
            a.out_inds[row] = i;
        }
        local += tot;
    }
}

// (min, first arg-min) of one cloud's potentials when it joins the table
__global__ __launch_bounds__(256) void sampler_cloud_min_kernel(const double* __restrict__ pot, long long p, double* out_min, long long* out_arg)
{
    __shared__ double sv[256];
    __shared__ long long si[256];
    double best = 1.0e308;
    long long bi = -1;
    for (long long i = threadIdx.x; i < p; i += 256) ws_argmin_take(best, bi, pot[i], i);
    ws_argmin_block(best, bi, sv, si);
    if (threadIdx.x == 0) { *out_min = sv[0]; *out_arg = si[0] < 0 ? 0 : si[0]; }
}

// ---- the class-balanced centre draw (DALES_PseudoLabel.py:961-975): np.where(labels == v)[0][pos] without the index list ----

// counts[(cloud * ncls + c) * gn + chunk] = members of class c (raw value values[c]) in that chunk of the cloud's labels
__global__ __launch_bounds__(256) void class_count_kernel(const WsCloud* __restrict__ clouds, const int32_t* __restrict__ values, int ncls,
                                                          int gn, int* __restrict__ counts)
{
    __shared__ int cnt[WS_SAMPLER_MAX_CLASSES];
    __shared__ int val[WS_SAMPLER_MAX_CLASSES];
    const int cloud = blockIdx.y, b = blockIdx.x;
    if (threadIdx.x < ncls) { cnt[threadIdx.x] = 0; val[threadIdx.x] = values[threadIdx.x]; }
    __syncthreads();
    const WsCloud cl = clouds[cloud];
    long long beg, end;
    chunk(cl.n, gn, b, beg, end);
    for (long long i = beg + threadIdx.x; i < end; i += 256) {
        const int l = cl.labels[i];
        for (int c = 0; c < ncls; ++c)
            if (val[c] == l) atomicAdd(&cnt[c], 1);        // integer, in LDS: the sum does not depend on the order
    }
    __syncthreads();
    if (threadIdx.x < ncls) counts[((long long)cloud * ncls + threadIdx.x) * gn + b] = cnt[threadIdx.x];
}

// one workgroup per cloud: every class's gn counts -> exclusive offsets in place, the class total -> totals[cloud, c]
__global__ __launch_bounds__(256) void class_scan_kernel(int ncls, int gn, int* __restrict__ counts, long long* __restrict__ totals)
{
    __shared__ int lds[WS_SCAN_BLOCK / 64 + 1];
    const int cloud = blockIdx.x;
    for (int c = 0; c < ncls; ++c) {
        int* row = counts + ((long long)cloud * ncls + c) * gn;
        int v[4], s = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = threadIdx.x * 4 + e;
            v[e] = j < gn ? row[j] : 0;
            s += v[e];
        }
        int total;
        int run = ws_block_exclusive_scan(s, lds, total);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = threadIdx.x * 4 + e;
            if (j < gn) row[j] = run;
            run += v[e];
        }
        if (threadIdx.x == 0) totals[(long long)cloud * ncls + c] = total;
    }
}

// one workgroup per (cloud, class, position): out = index of the position-th point of that class, ascending; -1 when the
// class has no such member (the labels changed since the counts were read)
__global__ __launch_bounds__(256) void class_select_kernel(const WsCloud* __restrict__ clouds, int nc, const int32_t* __restrict__ values,
                                                           int ncls, int gn, const int* __restrict__ offs,
                                                           const long long* __restrict__ triples, long long* __restrict__ out)
{
    __shared__ int lds[WS_SCAN_BLOCK / 64 + 1];
    const long long t = blockIdx.x;
    const long long cloud = triples[3 * t], c = triples[3 * t + 1], pos = triples[3 * t + 2];
    if (cloud < 0 || cloud >= nc || c < 0 || c >= ncls || pos < 0) return;
    const int* row = offs + (cloud * ncls + c) * gn;
    int lo = 0, hi = gn;                                   // last chunk whose offset is <= pos: empty chunks share the
    while (hi - lo > 1) {                                  // offset of the next one that holds a member
        const int mid = (lo + hi) >> 1;
        if (row[mid] <= pos) lo = mid; else hi = mid;
    }
    const WsCloud cl = clouds[cloud];
    const int v = values[c];
    long long beg, end;
    chunk(cl.n, gn, lo, beg, end);
    long long r = pos - row[lo];
    long long found = -1;
    for (long long t0 = beg; t0 < end; t0 += 256) {
        const long long i = t0 + threadIdx.x;
        const int f = (i < end && cl.labels[i] == v) ? 1 : 0;
        int tot;
        const int p = ws_block_exclusive_scan(f, lds, tot);
        if (r < tot) {
            if (f && p == r) found = i;
            break;
        }
        r -= tot;
    }
    if (found >= 0) out[t] = found;                        // `out` was filled with -1 before the launch
}

}  // namespace

struct ws_sampler {
    std::vector<WsCloud> clouds;
    WsCloud* d_clouds = nullptr;
    double* d_min = nullptr;
    long long* d_arg = nullptr;
    WsDraw* d_draws = nullptr;
    double* d_pv = nullptr;
    long long* d_pi = nullptr;
    int* d_counts = nullptr;
    int32_t* d_keep = nullptr;
    int* d_class = nullptr;            // per (cloud, class, chunk) counts of the centre draw, scanned in place
    size_t class_bytes = 0;
    int class_n = 0, class_gn = 0, class_nc = 0;
    long long nmax = 0, pmax = 0;
};

extern "C" {

int64_t ws_sampler_state_bytes(void) { return (int64_t)sizeof(WsState); }
int64_t ws_sampler_draw_bytes(void) { return (int64_t)sizeof(WsDraw); }

int ws_sampler_create(ws_sampler** out)
{
    WS_REQUIRE(out, "NULL argument");
    ws_sampler* ws = new ws_sampler();
    *out = ws;
    WS_HIP(hipMalloc(&ws->d_clouds, sizeof(WsCloud) * WS_SAMPLER_MAX_CLOUDS));
    WS_HIP(hipMalloc(&ws->d_min, sizeof(double) * WS_SAMPLER_MAX_CLOUDS));
    WS_HIP(hipMalloc(&ws->d_arg, sizeof(long long) * WS_SAMPLER_MAX_CLOUDS));
    WS_HIP(hipMalloc(&ws->d_draws, sizeof(WsDraw) * WS_SAMPLER_MAX_SPHERES));
    WS_HIP(hipMalloc(&ws->d_pv, sizeof(double) * WS_SAMPLER_GP));
    WS_HIP(hipMalloc(&ws->d_pi, sizeof(long long) * WS_SAMPLER_GP));
    WS_HIP(hipMalloc(&ws->d_counts, sizeof(int) * (WS_SAMPLER_GN + 1)));
    WS_HIP(hipMalloc(&ws->d_keep, sizeof(int32_t) * WS_SAMPLER_MAX_SPHERES));
    return WS_OK;
}

void ws_sampler_destroy(ws_sampler* ws)
{
    if (!ws) return;
    (void)hipFree(ws->d_clouds);
    (void)hipFree(ws->d_min);
    (void)hipFree(ws->d_arg);
    (void)hipFree(ws->d_draws);
    (void)hipFree(ws->d_pv);
    (void)hipFree(ws->d_pi);
    (void)hipFree(ws->d_counts);
    (void)hipFree(ws->d_keep);
    (void)hipFree(ws->d_class);
    delete ws;
}

int ws_sampler_add_cloud(ws_sampler* ws, const float* sub_points, const int32_t* sub_labels, int64_t n, const float* pot_points,
                         double* potentials, int64_t p, void* stream)
{
    const bool no_pot = !pot_points && !potentials && p == 0;      // a tile of the random mode: no potential is ever read
    WS_REQUIRE(ws && sub_points && (no_pot || (pot_points && potentials)), "NULL argument");
    WS_REQUIRE(n >= 1 && n < 2147483647ll && (no_pot || (p >= 1 && p < 2147483647ll)), "bad sizes n=%lld p=%lld", (long long)n,
               (long long)p);
    WS_REQUIRE(ws->clouds.size() < WS_SAMPLER_MAX_CLOUDS, "more than %d clouds", WS_SAMPLER_MAX_CLOUDS);
    const WsCloud cl{sub_points, sub_labels, pot_points, potentials, (long long)n, (long long)p, nullptr, 0};
    const size_t i = ws->clouds.size();
    hipStream_t st = (hipStream_t)stream;
    WS_HIP(hipMemcpyAsync(ws->d_clouds + i, &cl, sizeof(WsCloud), hipMemcpyHostToDevice, st));
    if (!no_pot) {
        sampler_cloud_min_kernel<<<1, 256, 0, st>>>(potentials, (long long)p, ws->d_min + i, ws->d_arg + i);
        WS_LAUNCH_CHECK();
    }
    WS_HIP(hipStreamSynchronize(st));                      // `cl` is a stack value
    ws->clouds.push_back(cl);
    if (n > ws->nmax) ws->nmax = n;
    if (p > ws->pmax) ws->pmax = p;
    return WS_OK;
}

int ws_sampler_set_colors(ws_sampler* ws, int32_t cloud, const float* colors, int32_t ncol, void* stream)
{
    WS_REQUIRE(ws && colors, "NULL argument");
    WS_REQUIRE(cloud >= 0 && (size_t)cloud < ws->clouds.size(), "cloud=%d outside [0, %d)", cloud, (int)ws->clouds.size());
    if (ncol < 1 || ncol > WS_SAMPLER_MAX_COLORS)
        return ws_fail(WS_ERR_UNSUPPORTED, "ncol=%d colour columns: 1 to %d are built", ncol, WS_SAMPLER_MAX_COLORS);
    WsCloud cl = ws->clouds[cloud];
    cl.colors = colors;
    cl.ncol = ncol;
    hipStream_t st = (hipStream_t)stream;
    WS_HIP(hipMemcpyAsync(ws->d_clouds + cloud, &cl, sizeof(WsCloud), hipMemcpyHostToDevice, st));
    WS_HIP(hipStreamSynchronize(st));                      // `cl` is a stack value
    ws->clouds[cloud] = cl;
    return WS_OK;
}

int64_t ws_sampler_items_bytes(void) { return (int64_t)sizeof(ws_sampler_items); }

int ws_sampler_batch_items(ws_sampler* ws, const ws_sampler_items* it)
{
    WS_REQUIRE(ws && it && it->h_draws && it->d_state, "NULL argument");
    WS_REQUIRE(!ws->clouds.empty(), "no cloud was added");
    const int32_t max_spheres = it->max_spheres, fd = it->fd;
    WS_REQUIRE(max_spheres >= 1 && max_spheres <= WS_SAMPLER_MAX_SPHERES, "max_spheres=%d outside [1, %d]", max_spheres,
               WS_SAMPLER_MAX_SPHERES);
    WS_REQUIRE(it->in_radius > 0.0 && it->capacity_rows >= 1 && it->batch_limit >= 0, "bad in_radius=%g capacity_rows=%lld batch_limit=%lld",
               it->in_radius, (long long)it->capacity_rows, (long long)it->batch_limit);
    const long long ncol = ws->clouds[0].ncol;
    for (const WsCloud& c : ws->clouds) WS_REQUIRE(c.ncol == ncol, "every cloud needs the same number of colour columns");
    if (ncol == 0) {
        if (fd != 1 && fd != 3) return ws_fail(WS_ERR_UNSUPPORTED, "Only accepted input dimensions are 1 and 3");
    } else if (fd != 1 && fd != 1 + ncol && fd != 3 + ncol) {
        return ws_fail(WS_ERR_UNSUPPORTED, "Only accepted input dimensions are 1, %d and %d", (int)(1 + ncol), (int)(3 + ncol));
    }
    WS_REQUIRE(it->out_points && it->out_features && it->out_labels && it->out_input_inds && it->out_lengths && it->out_scales &&
               it->out_rots && it->out_cloud_inds && it->out_point_inds, "NULL output");
    if (!it->labels_zero)
        for (const WsCloud& c : ws->clouds) WS_REQUIRE(c.labels, "a cloud without labels needs labels_zero");
    WS_REQUIRE(!it->label_lut || it->lut_n >= 1, "bad lut_n=%d", it->lut_n);
    if (it->random_centres) {
        WS_REQUIRE(it->epoch_inds && it->epoch_i && it->n_centres >= 1, "the random mode needs epoch_inds [2, n_centres >= 1] and epoch_i");
    } else {
        for (const WsCloud& c : ws->clouds) WS_REQUIRE(c.p >= 1, "a cloud without potential points serves the random mode only");
    }
    hipStream_t st = (hipStream_t)it->stream;
    WS_HIP(hipMemcpyAsync(ws->d_draws, it->h_draws, sizeof(WsDraw) * max_spheres, hipMemcpyHostToDevice, st));
    if (it->h_colour_keep)
        WS_HIP(hipMemcpyAsync(ws->d_keep, it->h_colour_keep, sizeof(int32_t) * max_spheres, hipMemcpyHostToDevice, st));
    WsArgs a;
    a.clouds = ws->d_clouds;
    a.nc = (int)ws->clouds.size();
    a.min_pot = ws->d_min;
    a.argmin = ws->d_arg;
    a.draws = ws->d_draws;
    a.st = (WsState*)it->d_state;
    a.pv = ws->d_pv;
    a.pi = ws->d_pi;
    a.counts = ws->d_counts;
    a.gp = (int)ws_ceil_div(ws->pmax, 256);
    if (a.gp > WS_SAMPLER_GP) a.gp = WS_SAMPLER_GP;
    if (it->random_centres) a.gp = 0;                      // no workgroup over the potential points
    a.gn = (int)ws_ceil_div(ws->nmax, 256);
    if (a.gn > WS_SAMPLER_GN) a.gn = WS_SAMPLER_GN;
    a.r2 = it->in_radius * it->in_radius;
    a.max_slots = max_spheres;
    a.batch_limit = it->batch_limit;
    a.capacity = it->capacity_rows;
    a.aug_noise = it->augment_noise;
    a.seed = it->seed;
    a.seq0 = it->seq0;
    a.fd = fd;
    a.lut = it->label_lut;
    a.lut_n = it->lut_n;
    a.labels_zero = it->labels_zero;
    a.update_pot = it->random_centres ? 0 : it->update_potentials;
    a.out_points = it->out_points;
    a.out_features = it->out_features;
    a.out_labels = (long long*)it->out_labels;
    a.out_inds = (long long*)it->out_input_inds;
    a.out_lengths = it->out_lengths;
    a.out_scales = it->out_scales;
    a.out_rots = it->out_rots;
    a.out_cloud_inds = it->out_cloud_inds;
    a.out_point_inds = it->out_point_inds;
    a.keep = it->h_colour_keep ? ws->d_keep : nullptr;
    a.ncol = (int)ncol;
    a.random = it->random_centres ? 1 : 0;
    a.epoch_inds = (const long long*)it->epoch_inds;
    a.n_centres = it->n_centres;
    a.epoch_i = (long long*)it->epoch_i;
    sampler_init_kernel<<<1, 256, 0, st>>>(a.st, it->resume);
    WS_LAUNCH_CHECK();
    for (int k = 0; k < max_spheres; ++k) {
        sphere_scan_kernel<<<a.gp + a.gn, 256, 0, st>>>(a);
        WS_LAUNCH_CHECK();
        sphere_decide_kernel<<<1, 256, 0, st>>>(a);
        WS_LAUNCH_CHECK();
        sphere_emit_kernel<<<a.gp + a.gn, 256, 0, st>>>(a);
        WS_LAUNCH_CHECK();
    }
    return WS_OK;
}

int ws_sampler_batch(ws_sampler* ws, const void* h_draws, int32_t max_spheres, int32_t resume, int64_t batch_limit, double in_radius,
                     float augment_noise, uint64_t seed, uint64_t seq0, int32_t fd, const int32_t* label_lut, int32_t lut_n,
                     int32_t labels_zero, int32_t update_potentials, float* out_points, float* out_features, int64_t* out_labels,
                     int64_t* out_input_inds, int32_t* out_lengths, float* out_scales, float* out_rots, int32_t* out_cloud_inds,
                     int32_t* out_point_inds, int64_t capacity_rows, void* d_state, void* stream)
{
    ws_sampler_items it = {};                              // no colour flags, centres from the potentials
    it.h_draws = h_draws;
    it.max_spheres = max_spheres;
    it.resume = resume;
    it.batch_limit = batch_limit;
    it.in_radius = in_radius;
    it.augment_noise = augment_noise;
    it.seed = seed;
    it.seq0 = seq0;
    it.fd = fd;
    it.label_lut = label_lut;
    it.lut_n = lut_n;
    it.labels_zero = labels_zero;
    it.update_potentials = update_potentials;
    it.out_points = out_points;
    it.out_features = out_features;
    it.out_labels = out_labels;
    it.out_input_inds = out_input_inds;
    it.out_lengths = out_lengths;
    it.out_scales = out_scales;
    it.out_rots = out_rots;
    it.out_cloud_inds = out_cloud_inds;
    it.out_point_inds = out_point_inds;
    it.capacity_rows = capacity_rows;
    it.d_state = d_state;
    it.stream = stream;
    return ws_sampler_batch_items(ws, &it);
}

/* the class-balanced centre draw, device half: see include/weasal_hip.h */
int ws_sampler_class_counts(ws_sampler* ws, const int32_t* values, int32_t n_class, int64_t* out_counts, void* stream)
{
    WS_REQUIRE(ws && values && out_counts, "NULL argument");
    WS_REQUIRE(!ws->clouds.empty(), "no cloud was added");
    WS_REQUIRE(n_class >= 1 && n_class <= WS_SAMPLER_MAX_CLASSES, "n_class=%d outside [1, %d]", n_class, WS_SAMPLER_MAX_CLASSES);
    for (const WsCloud& c : ws->clouds) WS_REQUIRE(c.labels, "the centre draw needs the labels of every cloud");
    const int nc = (int)ws->clouds.size();
    int gn = (int)ws_ceil_div(ws->nmax, 256);
    if (gn > WS_SAMPLER_GN) gn = WS_SAMPLER_GN;
    const size_t need = sizeof(int) * (size_t)nc * n_class * gn;
    if (need > ws->class_bytes) {
        WS_HIP(hipStreamSynchronize((hipStream_t)stream));
        (void)hipFree(ws->d_class);
        ws->d_class = nullptr;
        ws->class_bytes = 0;
        WS_HIP(hipMalloc(&ws->d_class, need));
        ws->class_bytes = need;
    }
    ws->class_n = n_class;
    ws->class_gn = gn;
    ws->class_nc = nc;
    hipStream_t st = (hipStream_t)stream;
    class_count_kernel<<<dim3(gn, nc), 256, 0, st>>>(ws->d_clouds, values, n_class, gn, ws->d_class);
    WS_LAUNCH_CHECK();
    class_scan_kernel<<<nc, 256, 0, st>>>(n_class, gn, ws->d_class, (long long*)out_counts);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_sampler_class_select(ws_sampler* ws, const int32_t* values, int32_t n_class, const int64_t* triples, int64_t n_triples,
                            int64_t* out_points, void* stream)
{
    WS_REQUIRE(ws && values && triples && out_points, "NULL argument");
    WS_REQUIRE(n_triples >= 1 && n_triples < 2147483647ll, "bad n_triples=%lld", (long long)n_triples);
    WS_REQUIRE(ws->d_class && ws->class_n == n_class && ws->class_nc == (int)ws->clouds.size(),
               "ws_sampler_class_select needs the ws_sampler_class_counts of the same classes and clouds first");
    hipStream_t st = (hipStream_t)stream;
    WS_HIP(hipMemsetAsync(out_points, 0xFF, sizeof(int64_t) * n_triples, st));     // -1: no such member
    class_select_kernel<<<(unsigned)n_triples, 256, 0, st>>>(ws->d_clouds, ws->class_nc, values, n_class, ws->class_gn, ws->d_class,
                                                             (const long long*)triples, (long long*)out_points);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

}  // extern "C"

