// weasal_amd/csrc/batchnorm.hip -- batch normalisation over the point axis of the stacked batch, with the residual sum and
// the LeakyReLU that follow it in the blocks (models/blocks.py:430-470: the BatchNormBlock whose nn.BatchNorm1d the reference
// constructs and, on [N, C] inputs, never runs; here it runs the way KPConv applies nn.BatchNorm1d).  gfx950 only.
//
//   ws_bn_fwd   training: bn_stats_kernel -> bn_finish_fwd_kernel -> bn_apply_fwd_kernel;  evaluation: bn_apply_fwd_kernel
//   ws_bn_bwd   bn_reduce_bwd_kernel -> bn_finish_bwd_kernel -> bn_apply_bwd_kernel
//   ws_bn_variant   the reporter; bn_plan is the ONE plan function of the three entries
//
// The same launch sequence CUT where a collective goes, for batch statistics over the rows of several ranks (the caller
// gathers the records between the entries; ops.batch_norm_act(group=...)):
//   ws_bn_moments          bn_stats_kernel -> bn_local_fwd_kernel: this rank's record [5, c] = n, sum, hi, lo, M2
//   ws_bn_moments_finish   bn_sync_finish_kernel: the gathered records [world, 5, c] merged in rank order, save_mean / save_rstd,
//                          the running statistics with the GLOBAL count, which it also leaves on the device (n_global)
//   ws_bn_apply            bn_apply_fwd_kernel with a given mean and rstd
//   ws_bn_bwd_sums         bn_reduce_bwd_kernel -> bn_finish_bwd_kernel: this rank's record [2, c] = sum dz, sum dz * xhat
//   ws_bn_bwd_apply        bn_sync_sums_kernel (the gathered records [world, 2, c] added in rank order) -> bn_apply_bwd_kernel
//                          with the global sums and the global count
//   ws_bn_sync_variant     their reporter, over the same bn_plan
// With one rank the cut sequence gives the bits of ws_bn_fwd / ws_bn_bwd: the local finish merges the chunks in the order of
// bn_finish_fwd_kernel, and a merge over one record is that record.
//
// Streaming kernels: threads = column groups (V = 4 floats, 16 bytes per lane, or V = 1) x row lanes; a workgroup owns
// a chunk of rows and a tile of up to 64 column groups.  The variance is CENTRED: a thread holds up to BN_T rows in
// registers, takes their mean, then the squares of the differences from it -- two passes over registers, one over memory --
// and every further combination (a thread's batches, the row lanes of a workgroup through LDS, the chunks in the finish
// kernel) is Chan's merge of (count, mean, M2).  A partial mean travels as TWO floats, hi + lo: hi is the mean of the
// partial's first batch as float32 rounds it, lo the mean of the differences from hi -- which are exact where the data
// crowd around hi -- so that the difference of two partial means, whose square enters M2, is known to the precision of
// the spread and not of the magnitude (at |mean| / std = 1e3 a single float loses 3 of its 7 digits there).  The mean
// that is REPORTED is the plain column sum over n, added up along the same tree: hi + lo carries an error of the order
// of eps * |hi - mean|, which at |mean| << std is more than the sum's.  float32
// throughout, no float atomics, every merge order is a function of the shapes: both directions are run-to-run
// bit-identical.
#include "ws_common.h"

namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_TILE = 64;          // column groups per workgroup at most: one wave reads 1 KiB of a row at V = 4
constexpr int BN_T = 8;              // rows a thread holds in registers at once (statistics), rows per thread of a full chunk
constexpr int BN_U = 4;              // rows in flight per thread in the apply and reduce passes
constexpr int BN_CAP = 1024;         // chunks at most: 4 workgroups per CU
constexpr int BN_FILL = 256;         // workgroups wanted before a thread gets more than one row
constexpr int BN_FC = 4;             // finish kernels: columns per workgroup
constexpr int BN_FL = 64;            // finish kernels: chunk lanes per column
constexpr int BN_MAX_C = 1 << 20;

// The launch plan of one call: a function of n, c, the pitches and the 16-byte alignment of the pointers, nothing else.
struct BnPlan {
    int v;               // floats per lane: 4 (16-byte accesses) or 1
    int ncg;             // column groups = ceil(c / v)
    int per;             // column groups per workgroup (the column tile, in groups)
    int lanes;           // row lanes per workgroup = 256 / per
    int ctiles;          // column tiles = grid.y
    int64_t rows;        // rows per chunk, a multiple of `lanes`
    int chunks;          // grid.x
    int depth;           // merge levels in the finish kernel: 0 one chunk, 1 a tree over the lanes, 2 a run per lane, then the tree
    int fin_blocks;      // finish grid
};

inline bool bn_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int64_t bn_rows(int64_t n, int lanes, int ctiles)
{
    int64_t t = n * ctiles / ((int64_t)BN_FILL * lanes);          // rows per thread: 1 until BN_FILL workgroups exist, BN_T at most
    t = t < 1 ? 1 : (t > BN_T ? BN_T : t);
    int64_t rows = t * lanes;
    if (ws_ceil_div(n, rows) > BN_CAP) rows = ws_ceil_div(ws_ceil_div(n, BN_CAP), lanes) * lanes;
    return rows;
}

static BnPlan bn_plan_v(int64_t n, int32_t c, int v)
{
    BnPlan p{};
    p.v = v;
    p.ncg = (c + v - 1) / v;
    p.per = p.ncg < BN_TILE ? p.ncg : BN_TILE;
    p.lanes = BN_THREADS / p.per;
    p.ctiles = (p.ncg + p.per - 1) / p.per;
    p.rows = bn_rows(n, p.lanes, p.ctiles);
    p.chunks = (int)ws_ceil_div(n, p.rows);
    p.depth = p.chunks <= 1 ? 0 : (p.chunks <= BN_FL ? 1 : 2);
    p.fin_blocks = (c + BN_FC - 1) / BN_FC;
    return p;
}

// ptrs / lds: every [n, c] tensor the call touches (NULL = absent)
static BnPlan bn_plan(int64_t n, int32_t c, const void* const* ptrs, const int64_t* lds, int count)
{
    bool vec = c % 4 == 0;
    for (int i = 0; i < count && vec; ++i)
        if (ptrs[i]) vec = bn_al16(ptrs[i]) && lds[i] % 4 == 0;
    return bn_plan_v(n, c, vec ? 4 : 1);
}

struct Moments {
    float n, sum, hi, lo, m2;      // mean = hi + lo for the merges, sum / n for the output
};
// Chan, Golub, LeVeque: the moments of the union of two samples; the union keeps a's hi
__device__ __forceinline__ Moments bn_merge(const Moments a, const Moments b)
{
    if (b.n == 0.0f) return a;
    if (a.n == 0.0f) return b;
    const float n = a.n + b.n, d = (b.hi - a.hi) + (b.lo - a.lo), f = b.n / n;
    return Moments{n, a.sum + b.sum, a.hi, a.lo + d * f, a.m2 + b.m2 + d * d * (a.n * f)};
}

__device__ __forceinline__ int bn_pow2_below(int lanes)      // the largest power of two below `lanes` (lanes >= 2)
{
    int s = 1;
    while (s * 2 < lanes) s *= 2;
    return s;
}

// ---------------------------------------------------------------------------------------------
// forward statistics: (sum, mean = hi + lo, M2) of every chunk and column -> psum / phi / plo / pm2 [chunks, c]
// ---------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(BN_THREADS) void bn_stats_kernel(const float* __restrict__ y, int64_t n, int c, int64_t ldy, int per,
                                                              int lanes, int64_t rows, float* __restrict__ psum,
                                                              float* __restrict__ phi, float* __restrict__ plo,
                                                              float* __restrict__ pm2)
{
    typedef float vec_t __attribute__((ext_vector_type(V)));
    __shared__ float sn[BN_THREADS], ss[BN_THREADS * V], sh[BN_THREADS * V], sl[BN_THREADS * V], s2[BN_THREADS * V];
    const int t = threadIdx.x, rl = t / per, cgl = t % per;
    const int ncg = (c + V - 1) / V;
    const int cg = (int)blockIdx.y * per + cgl, col = cg * V;
    const bool active = rl < lanes && cg < ncg;
    const int64_t beg = (int64_t)blockIdx.x * rows;
    const int64_t end = beg + rows < n ? beg + rows : n;
    float an = 0.0f, as[V], ah[V], al[V], a2[V];
#pragma unroll
    for (int e = 0; e < V; ++e) as[e] = ah[e] = al[e] = a2[e] = 0.0f;
    if (active) {
        for (int64_t r0 = beg + rl; r0 < end; r0 += (int64_t)BN_T * lanes) {
            const int64_t left = (end - r0 + lanes - 1) / lanes;
            const int nb = left < BN_T ? (int)left : BN_T;
            vec_t v[BN_T];
            const float* p = y + r0 * ldy + col;
#pragma unroll
            for (int j = 0; j < BN_T; ++j)
                if (j < nb) v[j] = *reinterpret_cast<const vec_t*>(p + (int64_t)j * lanes * ldy);
            const float fb = (float)nb;
            const float nn = an + fb, f = fb / nn;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float s = 0.0f;
#pragma unroll
                for (int j = 0; j < BN_T; ++j)
                    if (j < nb) s += v[j][e];
                const float hb = s / fb;
                as[e] += s;
                float r = 0.0f;
#pragma unroll
                for (int j = 0; j < BN_T; ++j)
                    if (j < nb) r += v[j][e] - hb;
                const float lb = r / fb;
                float q = 0.0f;
#pragma unroll
                for (int j = 0; j < BN_T; ++j)
                    if (j < nb) {
                        const float d = (v[j][e] - hb) - lb;
                        q += d * d;
                    }
                if (an == 0.0f) {
                    ah[e] = hb;
                    al[e] = lb;
                    a2[e] = q;
                } else {
                    const float d = (hb - ah[e]) + (lb - al[e]);
                    al[e] += d * f;
                    a2[e] += q + d * d * (an * f);
                }
            }
            an = nn;
        }
    }
    sn[t] = an;
#pragma unroll
    for (int e = 0; e < V; ++e) {
        ss[t * V + e] = as[e];
        sh[t * V + e] = ah[e];
        sl[t * V + e] = al[e];
        s2[t * V + e] = a2[e];
    }
    // the row lanes of a column group, pairwise: lane rl takes lane rl + s for s = 2^k, ..., 2, 1
    for (int s = lanes > 1 ? bn_pow2_below(lanes) : 0; s >= 1; s >>= 1) {
        __syncthreads();
        if (active && rl < s && rl + s < lanes) {
            const int o = t + s * per;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const Moments m = bn_merge(Moments{sn[t], ss[t * V + e], sh[t * V + e], sl[t * V + e], s2[t * V + e]},
                                           Moments{sn[o], ss[o * V + e], sh[o * V + e], sl[o * V + e], s2[o * V + e]});
                ss[t * V + e] = m.sum;
                sh[t * V + e] = m.hi;
                sl[t * V + e] = m.lo;
                s2[t * V + e] = m.m2;
                if (e == V - 1) sn[t] = m.n;
            }
        }
    }
    if (active && rl == 0) {
#pragma unroll
        for (int e = 0; e < V; ++e)
            if (col + e < c) {
                psum[(int64_t)blockIdx.x * c + col + e] = ss[t * V + e];
                phi[(int64_t)blockIdx.x * c + col + e] = sh[t * V + e];
                plo[(int64_t)blockIdx.x * c + col + e] = sl[t * V + e];
                pm2[(int64_t)blockIdx.x * c + col + e] = s2[t * V + e];
            }
    }
}

// ---------------------------------------------------------------------------------------------
// forward finish: the chunks of a column merged in a fixed order (a run of consecutive chunks per lane, then the lanes
// pairwise), save_mean / save_rstd, and the running statistics of nn.BatchNorm1d -- all on the device
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BN_THREADS) void bn_finish_fwd_kernel(const float* __restrict__ psum, const float* __restrict__ phi,
                                                                   const float* __restrict__ plo, const float* __restrict__ pm2,
                                                                   int64_t n, int c, int64_t rows, int chunks, float eps,
                                                                   float momentum, float* __restrict__ running_mean,
                                                                   float* __restrict__ running_var, long long* __restrict__ nbt,
                                                                   float* __restrict__ save_mean, float* __restrict__ save_rstd)
{
    __shared__ float sn[BN_THREADS], ss[BN_THREADS], sh[BN_THREADS], sl[BN_THREADS], s2[BN_THREADS];
    const int t = threadIdx.x, cl = t % BN_FC, lane = t / BN_FC;
    const int col = (int)blockIdx.x * BN_FC + cl;
    const int run = (chunks + BN_FL - 1) / BN_FL;
    Moments a{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (col < c) {
        const int jend = (lane + 1) * run < chunks ? (lane + 1) * run : chunks;
        for (int j = lane * run; j < jend; ++j) {
            const int64_t left = n - (int64_t)j * rows;
            const Moments b{(float)(left < rows ? left : rows), psum[(int64_t)j * c + col], phi[(int64_t)j * c + col],
                            plo[(int64_t)j * c + col], pm2[(int64_t)j * c + col]};
            a = bn_merge(a, b);
        }
    }
    sn[t] = a.n;
    ss[t] = a.sum;
    sh[t] = a.hi;
    sl[t] = a.lo;
    s2[t] = a.m2;
    for (int s = BN_FL / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (lane < s) {
            const int o = t + s * BN_FC;
            const Moments m = bn_merge(Moments{sn[t], ss[t], sh[t], sl[t], s2[t]}, Moments{sn[o], ss[o], sh[o], sl[o], s2[o]});
            sn[t] = m.n;
            ss[t] = m.sum;
            sh[t] = m.hi;
            sl[t] = m.lo;
            s2[t] = m.m2;
        }
    }
    if (lane == 0 && col < c) {
        const float fn = (float)n;
        const float mean = ss[t] / fn, var = s2[t] / fn;
        save_mean[col] = mean;
        save_rstd[col] = 1.0f / sqrtf(var + eps);
        running_mean[col] = (1.0f - momentum) * running_mean[col] + momentum * mean;
        running_var[col] = (1.0f - momentum) * running_var[col] + momentum * (var * (fn / (fn - 1.0f)));
    }
    if (blockIdx.x == 0 && t == 0 && nbt) *nbt += 1;
}

// ---------------------------------------------------------------------------------------------
// forward apply: out = act((y - mean) * rstd * gamma + beta [+ residual]);  stat2 is rstd (training: what the finish kernel
// wrote) or the running variance (evaluation: rstd = 1 / sqrt(var + eps) once per thread)
// ---------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(BN_THREADS) void bn_apply_fwd_kernel(const float* __restrict__ y, int64_t n, int c, int64_t ldy, int per,
                                                                  int lanes, int64_t rows, const float* __restrict__ mean,
                                                                  const float* __restrict__ stat2, int stat2_is_var, float eps,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  const float* __restrict__ residual, int64_t ldr, int act,
                                                                  float slope, float* __restrict__ out, int64_t ldo)
{
    typedef float vec_t __attribute__((ext_vector_type(V)));
    const int t = threadIdx.x, rl = t / per, cgl = t % per;
    const int ncg = (c + V - 1) / V;
    const int cg = (int)blockIdx.y * per + cgl, col = cg * V;
    if (rl >= lanes || cg >= ncg) return;
    const int64_t beg = (int64_t)blockIdx.x * rows;
    const int64_t end = beg + rows < n ? beg + rows : n;
    float mu[V], rs[V], ga[V], be[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const int cc = col + e < c ? col + e : c - 1;
        mu[e] = mean[cc];
        rs[e] = stat2_is_var ? 1.0f / sqrtf(stat2[cc] + eps) : stat2[cc];
        ga[e] = gamma[cc];
        be[e] = beta[cc];
    }
    for (int64_t r0 = beg + rl; r0 < end; r0 += (int64_t)BN_U * lanes) {
        const int64_t left = (end - r0 + lanes - 1) / lanes;
        const int nb = left < BN_U ? (int)left : BN_U;
        vec_t v[BN_U], w[BN_U];
#pragma unroll
        for (int j = 0; j < BN_U; ++j)
            if (j < nb) {
                const int64_t r = r0 + (int64_t)j * lanes;
                v[j] = *reinterpret_cast<const vec_t*>(y + r * ldy + col);
                if (residual) w[j] = *reinterpret_cast<const vec_t*>(residual + r * ldr + col);
            }
#pragma unroll
        for (int j = 0; j < BN_U; ++j)
            if (j < nb) {
                vec_t z;
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    float x = (v[j][e] - mu[e]) * rs[e];
                    x = x * ga[e] + be[e];
                    if (residual) x += w[j][e];
                    if (act) x = x > 0.0f ? x : x * slope;
                    z[e] = x;
                }
                *reinterpret_cast<vec_t*>(out + (r0 + (int64_t)j * lanes) * ldo + col) = z;
            }
    }
}

// ---------------------------------------------------------------------------------------------
// backward reduction: per chunk and column the sums of dz and of dz * xhat (dz = dout gated by the OUTPUT) -> p1 / p2
// [chunks, c], in ONE pass; a thread adds its rows in row order, the row lanes are added pairwise through LDS
// ---------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(BN_THREADS) void bn_reduce_bwd_kernel(const float* __restrict__ dout, int64_t lddo,
                                                                   const float* __restrict__ outp, int64_t ldo,
                                                                   const float* __restrict__ y, int64_t ldy, int64_t n, int c, int per,
                                                                   int lanes, int64_t rows, const float* __restrict__ mean,
                                                                   const float* __restrict__ stat2, int stat2_is_var, float eps,
                                                                   int act, float slope, float* __restrict__ p1, float* __restrict__ p2)
{
    typedef float vec_t __attribute__((ext_vector_type(V)));
    __shared__ float s1[BN_THREADS * V], s2[BN_THREADS * V];
    const int t = threadIdx.x, rl = t / per, cgl = t % per;
    const int ncg = (c + V - 1) / V;
    const int cg = (int)blockIdx.y * per + cgl, col = cg * V;
    const bool active = rl < lanes && cg < ncg;
    const int64_t beg = (int64_t)blockIdx.x * rows;
    const int64_t end = beg + rows < n ? beg + rows : n;
    float a1[V], a2[V];
#pragma unroll
    for (int e = 0; e < V; ++e) a1[e] = a2[e] = 0.0f;
    if (active) {
        float mu[V], rs[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const int cc = col + e < c ? col + e : c - 1;
            mu[e] = mean[cc];
            rs[e] = stat2_is_var ? 1.0f / sqrtf(stat2[cc] + eps) : stat2[cc];
        }
        for (int64_t r0 = beg + rl; r0 < end; r0 += (int64_t)BN_U * lanes) {
            const int64_t left = (end - r0 + lanes - 1) / lanes;
            const int nb = left < BN_U ? (int)left : BN_U;
            vec_t g[BN_U], o[BN_U], v[BN_U];
#pragma unroll
            for (int j = 0; j < BN_U; ++j)
                if (j < nb) {
                    const int64_t r = r0 + (int64_t)j * lanes;
                    g[j] = *reinterpret_cast<const vec_t*>(dout + r * lddo + col);
                    if (act) o[j] = *reinterpret_cast<const vec_t*>(outp + r * ldo + col);
                    v[j] = *reinterpret_cast<const vec_t*>(y + r * ldy + col);
                }
#pragma unroll
            for (int j = 0; j < BN_U; ++j)
                if (j < nb) {
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        float dz = g[j][e];
                        if (act) dz = o[j][e] > 0.0f ? dz : dz * slope;
                        a1[e] += dz;
                        a2[e] += dz * ((v[j][e] - mu[e]) * rs[e]);
                    }
                }
        }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
        s1[t * V + e] = a1[e];
        s2[t * V + e] = a2[e];
    }
    for (int s = lanes > 1 ? bn_pow2_below(lanes) : 0; s >= 1; s >>= 1) {
        __syncthreads();
        if (active && rl < s && rl + s < lanes) {
            const int o = t + s * per;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                s1[t * V + e] += s1[o * V + e];
                s2[t * V + e] += s2[o * V + e];
            }
        }
    }
    if (active && rl == 0) {
#pragma unroll
        for (int e = 0; e < V; ++e)
            if (col + e < c) {
                p1[(int64_t)blockIdx.x * c + col + e] = s1[t * V + e];
                p2[(int64_t)blockIdx.x * c + col + e] = s2[t * V + e];
            }
    }
}

// backward finish: dbeta = sum of p1, dgamma = sum of p2 over the chunks, in the order of the forward finish
__global__ __launch_bounds__(BN_THREADS) void bn_finish_bwd_kernel(const float* __restrict__ p1, const float* __restrict__ p2, int c,
                                                                   int chunks, float* __restrict__ dgamma, float* __restrict__ dbeta)
{
    __shared__ float s1[BN_THREADS], s2[BN_THREADS];
    const int t = threadIdx.x, cl = t % BN_FC, lane = t / BN_FC;
    const int col = (int)blockIdx.x * BN_FC + cl;
    const int run = (chunks + BN_FL - 1) / BN_FL;
    float a1 = 0.0f, a2 = 0.0f;
    if (col < c) {
        const int jend = (lane + 1) * run < chunks ? (lane + 1) * run : chunks;
        for (int j = lane * run; j < jend; ++j) {
            a1 += p1[(int64_t)j * c + col];
            a2 += p2[(int64_t)j * c + col];
        }
    }
    s1[t] = a1;
    s2[t] = a2;
    for (int s = BN_FL / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (lane < s) {
            s1[t] += s1[t + s * BN_FC];
            s2[t] += s2[t + s * BN_FC];
        }
    }
    if (lane == 0 && col < c) {
        dbeta[col] = s1[t];
        dgamma[col] = s2[t];
    }
}

// ---------------------------------------------------------------------------------------------
// backward apply: dy = gamma * rstd * (dz - dbeta / N - xhat * dgamma / N) (training), gamma * rstd * dz (evaluation);
// dresidual = dz when asked for
// ---------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(BN_THREADS) void bn_apply_bwd_kernel(const float* __restrict__ dout, int64_t lddo,
                                                                  const float* __restrict__ outp, int64_t ldo,
                                                                  const float* __restrict__ y, int64_t ldy, int64_t n, int c, int per,
                                                                  int lanes, int64_t rows, const float* __restrict__ mean,
                                                                  const float* __restrict__ stat2, int stat2_is_var, float eps,
                                                                  const float* __restrict__ gamma, const float* __restrict__ dgamma,
                                                                  const float* __restrict__ dbeta, int training, int act, float slope,
                                                                  float* __restrict__ dy, int64_t lddy, float* __restrict__ dres,
                                                                  int64_t lddr, const long long* __restrict__ n_stat)
{
    typedef float vec_t __attribute__((ext_vector_type(V)));
    const int t = threadIdx.x, rl = t / per, cgl = t % per;
    const int ncg = (c + V - 1) / V;
    const int cg = (int)blockIdx.y * per + cgl, col = cg * V;
    if (rl >= lanes || cg >= ncg) return;
    const int64_t beg = (int64_t)blockIdx.x * rows;
    const int64_t end = beg + rows < n ? beg + rows : n;
    float mu[V], rs[V], gr[V], k1[V], k2[V];
    const float fn = (float)(n_stat ? (int64_t)*n_stat : n);      // the rows the sums run over: this call's, or all ranks'
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const int cc = col + e < c ? col + e : c - 1;
        mu[e] = mean[cc];
        rs[e] = stat2_is_var ? 1.0f / sqrtf(stat2[cc] + eps) : stat2[cc];
        gr[e] = gamma[cc] * rs[e];
        k1[e] = training ? dbeta[cc] / fn : 0.0f;
        k2[e] = training ? dgamma[cc] / fn : 0.0f;
    }
    for (int64_t r0 = beg + rl; r0 < end; r0 += (int64_t)BN_U * lanes) {
        const int64_t left = (end - r0 + lanes - 1) / lanes;
        const int nb = left < BN_U ? (int)left : BN_U;
        vec_t g[BN_U], o[BN_U], v[BN_U];
#pragma unroll
        for (int j = 0; j < BN_U; ++j)
            if (j < nb) {
                const int64_t r = r0 + (int64_t)j * lanes;
                g[j] = *reinterpret_cast<const vec_t*>(dout + r * lddo + col);
                if (act) o[j] = *reinterpret_cast<const vec_t*>(outp + r * ldo + col);
                if (training) v[j] = *reinterpret_cast<const vec_t*>(y + r * ldy + col);
            }
#pragma unroll
        for (int j = 0; j < BN_U; ++j)
            if (j < nb) {
                const int64_t r = r0 + (int64_t)j * lanes;
                vec_t dz, d;
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    float z = g[j][e];
                    if (act) z = o[j][e] > 0.0f ? z : z * slope;
                    dz[e] = z;
                    d[e] = training ? gr[e] * (z - k1[e] - ((v[j][e] - mu[e]) * rs[e]) * k2[e]) : gr[e] * z;
                }
                *reinterpret_cast<vec_t*>(dy + r * lddy + col) = d;
                if (dres) *reinterpret_cast<vec_t*>(dres + r * lddr + col) = dz;
            }
    }
}

// ---------------------------------------------------------------------------------------------
// the cut sequence.  bn_local_fwd_kernel is bn_finish_fwd_kernel up to the merged moments of a column -- the same run per lane,
// the same tree, so the same bits -- and stops there: the record of this rank's rows.  (Its own copy of the tree, not a
// function shared with bn_finish_fwd_kernel: that kernel's code object stays what it was.)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BN_THREADS) void bn_local_fwd_kernel(const float* __restrict__ psum, const float* __restrict__ phi,
                                                                  const float* __restrict__ plo, const float* __restrict__ pm2,
                                                                  int64_t n, int c, int64_t rows, int chunks, float* __restrict__ rec)
{
    __shared__ float sn[BN_THREADS], ss[BN_THREADS], sh[BN_THREADS], sl[BN_THREADS], s2[BN_THREADS];
    const int t = threadIdx.x, cl = t % BN_FC, lane = t / BN_FC;
    const int col = (int)blockIdx.x * BN_FC + cl;
    const int run = (chunks + BN_FL - 1) / BN_FL;
    Moments a{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (col < c) {
        const int jend = (lane + 1) * run < chunks ? (lane + 1) * run : chunks;
        for (int j = lane * run; j < jend; ++j) {
            const int64_t left = n - (int64_t)j * rows;
            const Moments b{(float)(left < rows ? left : rows), psum[(int64_t)j * c + col], phi[(int64_t)j * c + col],
                            plo[(int64_t)j * c + col], pm2[(int64_t)j * c + col]};
            a = bn_merge(a, b);
        }
    }
    sn[t] = a.n;
    ss[t] = a.sum;
    sh[t] = a.hi;
    sl[t] = a.lo;
    s2[t] = a.m2;
    for (int s = BN_FL / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (lane < s) {
            const int o = t + s * BN_FC;
            const Moments m = bn_merge(Moments{sn[t], ss[t], sh[t], sl[t], s2[t]}, Moments{sn[o], ss[o], sh[o], sl[o], s2[o]});
            sn[t] = m.n;
            ss[t] = m.sum;
            sh[t] = m.hi;
            sl[t] = m.lo;
            s2[t] = m.m2;
        }
    }
    if (lane == 0 && col < c) {
        rec[col] = (float)n;      // exact: the entry takes up to 2^24 rows
        rec[(int64_t)c + col] = ss[t];
        rec[(int64_t)2 * c + col] = sh[t];
        rec[(int64_t)3 * c + col] = sl[t];
        rec[(int64_t)4 * c + col] = s2[t];
    }
}

// the records of all ranks [world, 5, c] -> save_mean / save_rstd and the running statistics of the union of their rows; a
// thread owns a column and merges the ranks in rank order.  N, the global count, is the integer sum of the records' counts; it
// goes to *n_global, and with N < 2 nothing else is written
__global__ __launch_bounds__(BN_THREADS) void bn_sync_finish_kernel(const float* __restrict__ rec, int world, int c, float eps,
                                                                    float momentum, float* __restrict__ running_mean,
                                                                    float* __restrict__ running_var, long long* __restrict__ nbt,
                                                                    float* __restrict__ save_mean, float* __restrict__ save_rstd,
                                                                    long long* __restrict__ n_global)
{
    const int col = (int)blockIdx.x * BN_THREADS + (int)threadIdx.x;
    if (col >= c) return;
    Moments a{rec[col], rec[(int64_t)c + col], rec[(int64_t)2 * c + col], rec[(int64_t)3 * c + col], rec[(int64_t)4 * c + col]};
    long long total = (long long)a.n;
    for (int r = 1; r < world; ++r) {
        const float* q = rec + (int64_t)r * 5 * c;
        const Moments b{q[col], q[(int64_t)c + col], q[(int64_t)2 * c + col], q[(int64_t)3 * c + col], q[(int64_t)4 * c + col]};
        total += (long long)b.n;
        a = bn_merge(a, b);
    }
    if (total >= 2) {
        const float fn = (float)total;
        const float mean = a.sum / fn, var = a.m2 / fn;
        save_mean[col] = mean;
        save_rstd[col] = 1.0f / sqrtf(var + eps);
        running_mean[col] = (1.0f - momentum) * running_mean[col] + momentum * mean;
        running_var[col] = (1.0f - momentum) * running_var[col] + momentum * (var * (fn / (fn - 1.0f)));
    }
    if (col == 0) {
        *n_global = total;
        if (total >= 2 && nbt) *nbt += 1;
    }
}

// the backward records of all ranks [world, 2, c] added in rank order -> sums [2, c]: sum dz, sum dz * xhat over all rows
__global__ __launch_bounds__(BN_THREADS) void bn_sync_sums_kernel(const float* __restrict__ rec, int world, int c,
                                                                  float* __restrict__ sums)
{
    const int col = (int)blockIdx.x * BN_THREADS + (int)threadIdx.x;
    if (col >= c) return;
    float a1 = rec[col], a2 = rec[(int64_t)c + col];
    for (int r = 1; r < world; ++r) {
        a1 += rec[(int64_t)r * 2 * c + col];
        a2 += rec[(int64_t)r * 2 * c + c + col];
    }
    sums[col] = a1;
    sums[(int64_t)c + col] = a2;
}

constexpr int64_t BN_SYNC_MAX_N = (int64_t)1 << 24;      // a record's count is a float: exact up to here
constexpr int BN_SYNC_MAX_WORLD = 1 << 16;

int bn_check_shape(int64_t n, int32_t c)
{
    WS_REQUIRE(n >= 0 && c >= 1, "bad shape n %lld c %d", (long long)n, c);
    if (c > BN_MAX_C) return ws_fail(WS_ERR_UNSUPPORTED, "batch norm takes up to %d columns (got %d)", BN_MAX_C, c);
    return WS_OK;
}

}  // namespace

extern "C" {

int64_t ws_bn_scratch_bytes(int64_t n, int32_t c)
{
    if (n < 0 || c < 1 || c > BN_MAX_C) return -1;
    if (n == 0) return 0;
    const int a = bn_plan_v(n, c, 1).chunks, b = bn_plan_v(n, c, 4).chunks;      // (the pointers decide between the two)
    return (int64_t)4 * (a > b ? a : b) * c * (int64_t)sizeof(float);      // forward: sum, hi, lo, M2; backward: two sums
}

int ws_bn_fwd(const float* y, int64_t n, int32_t c, int64_t ldy, const float* gamma, const float* beta, float eps, int32_t training,
              float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked, const float* residual,
              int64_t ldr, int32_t act, float slope, float* out, int64_t ldo, float* save_mean, float* save_rstd, void* scratch,
              void* stream)
{
    if (int rc = bn_check_shape(n, c)) return rc;
    WS_REQUIRE(ldy >= c && ldo >= c && (!residual || ldr >= c), "row stride below the width %d", c);
    WS_REQUIRE(act == 0 || act == 1, "act %d: 0 none, 1 LeakyReLU", act);
    WS_REQUIRE(eps >= 0.0f, "negative eps");
    WS_REQUIRE(!training || n != 1, "training statistics need more than 1 row (torch: 'Expected more than 1 value per channel')");
    if (n == 0) return WS_OK;
    WS_REQUIRE(y && gamma && beta && out && running_mean && running_var, "NULL argument");
    WS_REQUIRE(!training || (save_mean && save_rstd && scratch), "training needs save_mean, save_rstd and scratch");
    const void* ptrs[3] = {y, out, residual};
    const int64_t lds[3] = {ldy, ldo, ldr};
    const BnPlan p = bn_plan(n, c, ptrs, lds, 3);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(p.chunks, p.ctiles);
    if (training) {
        float* psum = (float*)scratch;
        float* phi = psum + (int64_t)p.chunks * c;
        float* plo = phi + (int64_t)p.chunks * c;
        float* pm2 = plo + (int64_t)p.chunks * c;
        if (p.v == 4) bn_stats_kernel<4><<<grid, BN_THREADS, 0, st>>>(y, n, c, ldy, p.per, p.lanes, p.rows, psum, phi, plo, pm2);
        else bn_stats_kernel<1><<<grid, BN_THREADS, 0, st>>>(y, n, c, ldy, p.per, p.lanes, p.rows, psum, phi, plo, pm2);
        WS_LAUNCH_CHECK();
        bn_finish_fwd_kernel<<<p.fin_blocks, BN_THREADS, 0, st>>>(psum, phi, plo, pm2, n, c, p.rows, p.chunks, eps, momentum, running_mean,
                                                                  running_var, (long long*)num_batches_tracked, save_mean, save_rstd);
        WS_LAUNCH_CHECK();
    }
    const float* mean = training ? save_mean : running_mean;
    const float* stat2 = training ? save_rstd : running_var;
    if (p.v == 4)
        bn_apply_fwd_kernel<4><<<grid, BN_THREADS, 0, st>>>(y, n, c, ldy, p.per, p.lanes, p.rows, mean, stat2, training ? 0 : 1, eps, gamma,
                                                            beta, residual, ldr, act, slope, out, ldo);
    else
        bn_apply_fwd_kernel<1><<<grid, BN_THREADS, 0, st>>>(y, n, c, ldy, p.per, p.lanes, p.rows, mean, stat2, training ? 0 : 1, eps, gamma,
                                                            beta, residual, ldr, act, slope, out, ldo);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_bn_bwd(const float* dout, int64_t lddo, const float* out, int64_t ldo, const float* y, int64_t ldy, int64_t n, int32_t c,
              const float* gamma, const float* save_mean, const float* save_rstd, const float* running_mean,
              const float* running_var, float eps, int32_t training, int32_t act, float slope, float* dy, int64_t lddy,
              float* dresidual, int64_t lddr, float* dgamma, float* dbeta, void* scratch, void* stream)
{
    if (int rc = bn_check_shape(n, c)) return rc;
    WS_REQUIRE(lddo >= c && ldy >= c && lddy >= c && (!act || ldo >= c) && (!dresidual || lddr >= c), "row stride below the width %d", c);
    WS_REQUIRE(act == 0 || act == 1, "act %d: 0 none, 1 LeakyReLU", act);
    WS_REQUIRE(eps >= 0.0f, "negative eps");
    WS_REQUIRE(!training || n != 1, "training statistics need more than 1 row");
    WS_REQUIRE(dgamma && dbeta, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        WS_HIP(hipMemsetAsync(dgamma, 0, sizeof(float) * (size_t)c, st));
        WS_HIP(hipMemsetAsync(dbeta, 0, sizeof(float) * (size_t)c, st));
        return WS_OK;
    }
    WS_REQUIRE(dout && y && gamma && dy && scratch && (!act || out), "NULL argument");
    WS_REQUIRE(training ? (save_mean && save_rstd) : (running_mean && running_var),
               "training needs save_mean / save_rstd, evaluation running_mean / running_var");
    const void* ptrs[5] = {dout, act ? out : nullptr, y, dy, dresidual};
    const int64_t lds[5] = {lddo, ldo, ldy, lddy, lddr};
    const BnPlan p = bn_plan(n, c, ptrs, lds, 5);
    const dim3 grid(p.chunks, p.ctiles);
    float* p1 = (float*)scratch;
    float* p2 = p1 + (int64_t)p.chunks * c;
    const float* mean = training ? save_mean : running_mean;
    const float* stat2 = training ? save_rstd : running_var;
    const int isvar = training ? 0 : 1;
    if (p.v == 4)
        bn_reduce_bwd_kernel<4><<<grid, BN_THREADS, 0, st>>>(dout, lddo, out, ldo, y, ldy, n, c, p.per, p.lanes, p.rows, mean, stat2, isvar,
                                                             eps, act, slope, p1, p2);
    else
        bn_reduce_bwd_kernel<1><<<grid, BN_THREADS, 0, st>>>(dout, lddo, out, ldo, y, ldy, n, c, p.per, p.lanes, p.rows, mean, stat2, isvar,
                                                             eps, act, slope, p1, p2);
    WS_LAUNCH_CHECK();
    bn_finish_bwd_kernel<<<p.fin_blocks, BN_THREADS, 0, st>>>(p1, p2, c, p.chunks, dgamma, dbeta);
    WS_LAUNCH_CHECK();
    if (p.v == 4)
        bn_apply_bwd_kernel<4><<<grid, BN_THREADS, 0, st>>>(dout, lddo, out, ldo, y, ldy, n, c, p.per, p.lanes, p.rows, mean, stat2, isvar, eps,
                                                            gamma, dgamma, dbeta, training ? 1 : 0, act, slope, dy, lddy, dresidual, lddr, nullptr);
    else
        bn_apply_bwd_kernel<1><<<grid, BN_THREADS, 0, st>>>(dout, lddo, out, ldo, y, ldy, n, c, p.per, p.lanes, p.rows, mean, stat2, isvar, eps,
                                                            gamma, dgamma, dbeta, training ? 1 : 0, act, slope, dy, lddy, dresidual, lddr, nullptr);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_bn_variant(int32_t backward, int64_t n, int32_t c, const void* y, int64_t ldy, const void* out, int64_t ldo,
                  const void* residual, int64_t ldr, const void* dout, int64_t lddo, const void* dy, int64_t lddy, int32_t training,
                  int32_t act, char* text, int32_t cap)
{
    WS_REQUIRE(text && cap > 0, "bad argument");
    if (int rc = bn_check_shape(n, c)) return rc;
    WS_REQUIRE(!training || n != 1, "training statistics need more than 1 row");
    if (n == 0) {
        snprintf(text, (size_t)cap, "%s (n == 0)", backward ? "memset" : "none");
        return WS_OK;
    }
    BnPlan p;
    if (backward) {
        const void* ptrs[5] = {dout, act ? out : nullptr, y, dy, residual};
        const int64_t lds[5] = {lddo, ldo, ldy, lddy, ldr};
        p = bn_plan(n, c, ptrs, lds, 5);
    } else {
        const void* ptrs[3] = {y, out, residual};
        const int64_t lds[3] = {ldy, ldo, ldr};
        p = bn_plan(n, c, ptrs, lds, 3);
    }
    const char* kernels = backward ? "bn_reduce_bwd_kernel+bn_finish_bwd_kernel+bn_apply_bwd_kernel"
                                   : (training ? "bn_stats_kernel+bn_finish_fwd_kernel+bn_apply_fwd_kernel" : "bn_apply_fwd_kernel");
    const bool merges = backward || training;
    snprintf(text, (size_t)cap, "%s<V=%d> %s rows=%lld chunks=%d depth=%d tile=%d lanes=%d ctiles=%d mode=%s residual=%d act=%d", kernels,
             p.v, p.v == 4 ? "vector" : "scalar", (long long)p.rows, p.chunks, merges ? p.depth : 0, p.per * p.v, p.lanes, p.ctiles,
             training ? "training" : "evaluation", residual ? 1 : 0, act ? 1 : 0);
    return WS_OK;
}

int ws_bn_moments(const float* y, int64_t n, int32_t c, int64_t ldy, float* record, void* scratch, void* stream)
{
    if (int rc = bn_check_shape(n, c)) return rc;
    WS_REQUIRE(ldy >= c, "row stride below the width %d", c);
    WS_REQUIRE(record, "NULL argument");
    if (n > BN_SYNC_MAX_N)
        return ws_fail(WS_ERR_UNSUPPORTED, "a record counts up to %lld rows of one rank (got %lld)", (long long)BN_SYNC_MAX_N, (long long)n);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        WS_HIP(hipMemsetAsync(record, 0, sizeof(float) * 5 * (size_t)c, st));
        return WS_OK;
    }
    WS_REQUIRE(y && scratch, "NULL argument");
    const void* ptrs[1] = {y};
    const int64_t lds[1] = {ldy};
    const BnPlan p = bn_plan(n, c, ptrs, lds, 1);
    const dim3 grid(p.chunks, p.ctiles);
    float* psum = (float*)scratch;
    float* phi = psum + (int64_t)p.chunks * c;
    float* plo = phi + (int64_t)p.chunks * c;
    float* pm2 = plo + (int64_t)p.chunks * c;
    if (p.v == 4) bn_stats_kernel<4><<<grid, BN_THREADS, 0, st>>>(y, n, c, ldy, p.per, p.lanes, p.rows, psum, phi, plo, pm2);
    else bn_stats_kernel<1><<<grid, BN_THREADS, 0, st>>>(y, n, c, ldy, p.per, p.lanes, p.rows, psum, phi, plo, pm2);
    WS_LAUNCH_CHECK();
    bn_local_fwd_kernel<<<p.fin_blocks, BN_THREADS, 0, st>>>(psum, phi, plo, pm2, n, c, p.rows, p.chunks, record);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_bn_moments_finish(const float* records, int32_t world, int32_t c, float eps, float momentum, float* running_mean,
                         float* running_var, int64_t* num_batches_tracked, float* save_mean, float* save_rstd, int64_t* n_global,
                         void* stream)
{
    if (int rc = bn_check_shape(0, c)) return rc;
    WS_REQUIRE(world >= 1 && world <= BN_SYNC_MAX_WORLD, "world %d: 1 .. %d ranks", world, BN_SYNC_MAX_WORLD);
    WS_REQUIRE(eps >= 0.0f, "negative eps");
    WS_REQUIRE(records && running_mean && running_var && save_mean && save_rstd && n_global, "NULL argument");
    bn_sync_finish_kernel<<<(c + BN_THREADS - 1) / BN_THREADS, BN_THREADS, 0, (hipStream_t)stream>>>(
        records, world, c, eps, momentum, running_mean, running_var, (long long*)num_batches_tracked, save_mean, save_rstd,
        (long long*)n_global);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_bn_apply(const float* y, int64_t n, int32_t c, int64_t ldy, const float* mean, const float* rstd, const float* gamma,
                const float* beta, const float* residual, int64_t ldr, int32_t act, float slope, float* out, int64_t ldo, void* stream)
{
    if (int rc = bn_check_shape(n, c)) return rc;
    WS_REQUIRE(ldy >= c && ldo >= c && (!residual || ldr >= c), "row stride below the width %d", c);
    WS_REQUIRE(act == 0 || act == 1, "act %d: 0 none, 1 LeakyReLU", act);
    if (n == 0) return WS_OK;
    WS_REQUIRE(y && mean && rstd && gamma && beta && out, "NULL argument");
    const void* ptrs[3] = {y, out, residual};
    const int64_t lds[3] = {ldy, ldo, ldr};
    const BnPlan p = bn_plan(n, c, ptrs, lds, 3);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(p.chunks, p.ctiles);
    if (p.v == 4)
        bn_apply_fwd_kernel<4><<<grid, BN_THREADS, 0, st>>>(y, n, c, ldy, p.per, p.lanes, p.rows, mean, rstd, 0, 0.0f, gamma, beta, residual,
                                                            ldr, act, slope, out, ldo);
    else
        bn_apply_fwd_kernel<1><<<grid, BN_THREADS, 0, st>>>(y, n, c, ldy, p.per, p.lanes, p.rows, mean, rstd, 0, 0.0f, gamma, beta, residual,
                                                            ldr, act, slope, out, ldo);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_bn_bwd_sums(const float* dout, int64_t lddo, const float* out, int64_t ldo, const float* y, int64_t ldy, int64_t n, int32_t c,
                   const float* save_mean, const float* save_rstd, int32_t act, float slope, float* record, void* scratch, void* stream)
{
    if (int rc = bn_check_shape(n, c)) return rc;
    WS_REQUIRE(lddo >= c && ldy >= c && (!act || ldo >= c), "row stride below the width %d", c);
    WS_REQUIRE(act == 0 || act == 1, "act %d: 0 none, 1 LeakyReLU", act);
    WS_REQUIRE(record, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        WS_HIP(hipMemsetAsync(record, 0, sizeof(float) * 2 * (size_t)c, st));
        return WS_OK;
    }
    WS_REQUIRE(dout && y && save_mean && save_rstd && scratch && (!act || out), "NULL argument");
    const void* ptrs[3] = {dout, act ? out : nullptr, y};
    const int64_t lds[3] = {lddo, ldo, ldy};
    const BnPlan p = bn_plan(n, c, ptrs, lds, 3);
    const dim3 grid(p.chunks, p.ctiles);
    float* p1 = (float*)scratch;
    float* p2 = p1 + (int64_t)p.chunks * c;
    if (p.v == 4)
        bn_reduce_bwd_kernel<4><<<grid, BN_THREADS, 0, st>>>(dout, lddo, out, ldo, y, ldy, n, c, p.per, p.lanes, p.rows, save_mean, save_rstd,
                                                             0, 0.0f, act, slope, p1, p2);
    else
        bn_reduce_bwd_kernel<1><<<grid, BN_THREADS, 0, st>>>(dout, lddo, out, ldo, y, ldy, n, c, p.per, p.lanes, p.rows, save_mean, save_rstd,
                                                             0, 0.0f, act, slope, p1, p2);
    WS_LAUNCH_CHECK();
    bn_finish_bwd_kernel<<<p.fin_blocks, BN_THREADS, 0, st>>>(p1, p2, c, p.chunks, record + c, record);      // (dgamma, dbeta)
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_bn_bwd_apply(const float* dout, int64_t lddo, const float* out, int64_t ldo, const float* y, int64_t ldy, int64_t n, int32_t c,
                    const float* gamma, const float* save_mean, const float* save_rstd, const float* records, int32_t world,
                    const int64_t* n_global, int32_t act, float slope, float* dy, int64_t lddy, float* dresidual, int64_t lddr,
                    void* scratch, void* stream)
{
    if (int rc = bn_check_shape(n, c)) return rc;
    WS_REQUIRE(lddo >= c && ldy >= c && lddy >= c && (!act || ldo >= c) && (!dresidual || lddr >= c), "row stride below the width %d", c);
    WS_REQUIRE(act == 0 || act == 1, "act %d: 0 none, 1 LeakyReLU", act);
    WS_REQUIRE(world >= 1 && world <= BN_SYNC_MAX_WORLD, "world %d: 1 .. %d ranks", world, BN_SYNC_MAX_WORLD);
    if (n == 0) return WS_OK;
    WS_REQUIRE(dout && y && gamma && save_mean && save_rstd && records && n_global && dy && scratch && (!act || out), "NULL argument");
    const void* ptrs[5] = {dout, act ? out : nullptr, y, dy, dresidual};
    const int64_t lds[5] = {lddo, ldo, ldy, lddy, lddr};
    const BnPlan p = bn_plan(n, c, ptrs, lds, 5);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(p.chunks, p.ctiles);
    float* sums = (float*)scratch;      // [2, c]: within ws_bn_scratch_bytes for any n >= 1
    bn_sync_sums_kernel<<<(c + BN_THREADS - 1) / BN_THREADS, BN_THREADS, 0, st>>>(records, world, c, sums);
    WS_LAUNCH_CHECK();
    const long long* ng = (const long long*)n_global;
    if (p.v == 4)
        bn_apply_bwd_kernel<4><<<grid, BN_THREADS, 0, st>>>(dout, lddo, out, ldo, y, ldy, n, c, p.per, p.lanes, p.rows, save_mean, save_rstd, 0,
                                                            0.0f, gamma, sums + c, sums, 1, act, slope, dy, lddy, dresidual, lddr, ng);
    else
        bn_apply_bwd_kernel<1><<<grid, BN_THREADS, 0, st>>>(dout, lddo, out, ldo, y, ldy, n, c, p.per, p.lanes, p.rows, save_mean, save_rstd, 0,
                                                            0.0f, gamma, sums + c, sums, 1, act, slope, dy, lddy, dresidual, lddr, ng);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_bn_sync_variant(int32_t stage, int64_t n, int32_t c, int32_t world, const void* y, int64_t ldy, const void* out, int64_t ldo,
                       const void* residual, int64_t ldr, const void* dout, int64_t lddo, const void* dy, int64_t lddy, int32_t act,
                       char* text, int32_t cap)
{
    WS_REQUIRE(text && cap > 0, "bad argument");
    WS_REQUIRE(stage >= 0 && stage <= 4, "stage %d: 0 moments, 1 moments_finish, 2 apply, 3 bwd_sums, 4 bwd_apply", stage);
    if (int rc = bn_check_shape(n, c)) return rc;
    if (stage == 1) {
        WS_REQUIRE(world >= 1 && world <= BN_SYNC_MAX_WORLD, "world %d: 1 .. %d ranks", world, BN_SYNC_MAX_WORLD);
        snprintf(text, (size_t)cap, "bn_sync_finish_kernel world=%d blocks=%d", world, (c + BN_THREADS - 1) / BN_THREADS);
        return WS_OK;
    }
    if (n == 0) {
        snprintf(text, (size_t)cap, "%s (n == 0)", stage == 0 || stage == 3 ? "memset" : "none");
        return WS_OK;
    }
    const void* ptrs[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int64_t lds[5] = {0, 0, 0, 0, 0};
    const char* kernels = "";
    if (stage == 0) {
        if (n > BN_SYNC_MAX_N) return ws_fail(WS_ERR_UNSUPPORTED, "a record counts up to %lld rows of one rank", (long long)BN_SYNC_MAX_N);
        ptrs[0] = y, lds[0] = ldy;
        kernels = "bn_stats_kernel+bn_local_fwd_kernel";
    } else if (stage == 2) {
        ptrs[0] = y, lds[0] = ldy, ptrs[1] = out, lds[1] = ldo, ptrs[2] = residual, lds[2] = ldr;
        kernels = "bn_apply_fwd_kernel";
    } else {
        ptrs[0] = dout, lds[0] = lddo, ptrs[1] = act ? out : nullptr, lds[1] = ldo, ptrs[2] = y, lds[2] = ldy;
        if (stage == 4) ptrs[3] = dy, lds[3] = lddy, ptrs[4] = residual, lds[4] = ldr;
        kernels = stage == 3 ? "bn_reduce_bwd_kernel+bn_finish_bwd_kernel" : "bn_sync_sums_kernel+bn_apply_bwd_kernel";
    }
    const BnPlan p = bn_plan(n, c, ptrs, lds, 5);
    const bool merges = stage == 0 || stage == 3;
    snprintf(text, (size_t)cap, "%s<V=%d> %s rows=%lld chunks=%d depth=%d tile=%d lanes=%d ctiles=%d world=%d residual=%d act=%d", kernels,
             p.v, p.v == 4 ? "vector" : "scalar", (long long)p.rows, p.chunks, merges ? p.depth : 0, p.per * p.v, p.lanes, p.ctiles, world,
             residual ? 1 : 0, act ? 1 : 0);
    return WS_OK;
}

}  // extern "C"
