// weasal_amd/csrc/active.hip -- the active-learning selection that follows a voting pass over the training clouds: from the
// votes resident in HBM to the ids of the next ground-truth labels, without a host copy of the [N, C] probabilities.
//
//   ws_al_point_scores   utils/tester_PseudoLabel.py:400-414 : entropy of every sub-cloud point (float32, like numpy on the
//                        float32 votes), arg-max class, entropy * exp(class_w[arg-max]) as float64
//   ws_al_anchor_scores  utils/tester_WeakLabel.py:436-454 : per anchor, mean entropy of its points times the sum of the
//                        class scores of the classes predicted inside it
//   ws_topk_select       tester_PseudoLabel.py:416-429 / tester_WeakLabel.py:456-465 : argsort(-score), drop the used ids,
//                        keep the first k -- as an exact selection: order-preserving 64-bit keys, a most-significant-digit
//                        radix select of the k-th key, a compaction in index order (ws_scan.h) and a stable least-
//                        significant-digit radix sort of the k survivors.  The reference removes the used ids with one
//                        np.delete(np.where()) per id, O(used * N); here they are a bitmap and cost nothing per id.
//   ws_al_spaced_select  no counterpart in the reference (opt-in, `al_min_spacing`): the greedy walk over the candidates in
//                        ws_topk_select's order that accepts a candidate only when it keeps a minimum distance to every
//                        point accepted before it and to every used point; float64 distances, exact and run-to-run equal
// Order contract: descending score, ascending index among equal scores (stable), -0.0 == +0.0, NaN below every number.
#include "ws_common.h"
#include "ws_scan.h"
#include <vector>

namespace {

typedef unsigned long long u64;

constexpr int AL_ROWS = 256;              // rows of probs per workgroup tile (point scores)
constexpr int TK_SORT_CHUNK = 2048;       // survivors per single-wave workgroup of the sort passes
constexpr int TK_STATE_WORDS = 8 * 256;   // select histograms (uint32), followed by { prefix, k_rem } as 64-bit words

// ---------------------------------------------------------------------------------------------------------------------
// scores
// ---------------------------------------------------------------------------------------------------------------------
// One thread per row; the tile of AL_ROWS rows is staged in LDS with coalesced loads (a row is c * 4 bytes, 36 for the
// nine Vaihingen classes: a thread walking its own row in global memory would touch a line per load).  Row stride c | 1:
// odd, so that the 64 lanes of a wave fall on different banks.
__global__ __launch_bounds__(AL_ROWS) void point_scores_kernel(const float* __restrict__ probs, int64_t n, int c,
                                                               const double* __restrict__ class_score,
                                                               float* __restrict__ entropy, int32_t* __restrict__ preds,
                                                               double* __restrict__ score)
{
    extern __shared__ float tile[];
    const int ld = c | 1;
    const int64_t tiles = (n + AL_ROWS - 1) / AL_ROWS;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t r0 = t * AL_ROWS;
        const int rows = (int)(n - r0 < AL_ROWS ? n - r0 : AL_ROWS);
        const float* src = probs + r0 * c;
        for (int e = threadIdx.x; e < rows * c; e += AL_ROWS) tile[(e / c) * ld + (e % c)] = src[e];
        __syncthreads();
        if ((int)threadIdx.x < rows) {
            const float* p = tile + threadIdx.x * ld;
            float acc = 0.0f, bv = p[0];
            int best = 0;
            for (int k = 0; k < c; ++k) {                      // column order, like the reference's row sum
                const float pk = p[k];
                acc += pk * log2f(pk + 1e-12f);                 // product rounded, then added (-ffp-contract=off)
                if (k > 0 && pk > bv) { bv = pk; best = k; }    // first maximum (np.argmax)
            }
            const float h = 0.0f - acc;                        // a row without votes: +0, not -0
            entropy[r0 + threadIdx.x] = h;
            preds[r0 + threadIdx.x] = best;
            score[r0 + threadIdx.x] = (double)h * class_score[best];
        }
        __syncthreads();
    }
}

// one wave per anchor: f32 sum of the entropies, OR of the predicted-class bits
__global__ __launch_bounds__(256) void anchor_scores_kernel(const float* __restrict__ entropy, const int32_t* __restrict__ preds,
                                                            int64_t n, const int64_t* __restrict__ anchor_ptr,
                                                            const int64_t* __restrict__ anchor_idx, int64_t nnz, int64_t na,
                                                            const double* __restrict__ class_score, int c,
                                                            float* __restrict__ out)
{
    const int lane = ws_lane(), wave = threadIdx.x >> 6;
    for (int64_t a = (int64_t)blockIdx.x * 4 + wave; a < na; a += (int64_t)gridDim.x * 4) {
        int64_t beg = anchor_ptr[a], end = anchor_ptr[a + 1];
        if (beg < 0) beg = 0;
        if (end > nnz) end = nnz;
        float s = 0.0f;
        unsigned mask = 0u;
        for (int64_t e = beg + lane; e < end; e += 64) {
            const int64_t i = anchor_idx[e];
            if (i < 0 || i >= n) continue;
            s += entropy[i];
            const int p = preds[i];
            if (p >= 0 && p < c) mask |= 1u << p;
        }
        s = ws_wave_sum(s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mask |= (unsigned)__shfl_xor((int)mask, o, 64);
        if (lane == 0) {
            double cs = 0.0;
            for (int k = 0; k < c; ++k)
                if (mask >> k & 1u) cs += class_score[k];
            out[a] = end > beg ? (float)((double)(s / (float)(end - beg)) * cs) : 0.0f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// exact top-k
// ---------------------------------------------------------------------------------------------------------------------
// larger key = earlier in the selection.  0: an excluded id, 1: NaN, >= 2^52 - 1: every number (-inf maps to 2^52 - 1).
__device__ __forceinline__ u64 order_key(double x)
{
    if (x != x) return 1ull;
    if (x == 0.0) return 1ull << 63;                           // -0.0 and +0.0 share a key
    const u64 u = (u64)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}

__global__ __launch_bounds__(256) void topk_init_kernel(unsigned* __restrict__ state, long long k)
{
    for (int e = threadIdx.x; e < TK_STATE_WORDS; e += 256) state[e] = 0u;
    if (threadIdx.x == 0) {
        u64* s = (u64*)(state + TK_STATE_WORDS);
        s[0] = 0ull;                 // prefix of the k-th key found so far
        s[1] = (u64)k;               // rank of the k-th key among the keys that share the prefix
    }
}

__global__ __launch_bounds__(256) void topk_keys_kernel(const double* __restrict__ score, int64_t n,
                                                        const unsigned* __restrict__ excluded, u64* __restrict__ keys)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        keys[i] = (excluded[i >> 5] >> (i & 31) & 1u) ? 0ull : order_key(score[i]);
}

// histogram of the digit at `shift` over the keys that share the prefix above it.  Scores cluster (one exponent, one top
// byte): a thread counts runs of equal digits in a register and touches the LDS histogram only when the digit changes.
__global__ __launch_bounds__(256) void topk_select_hist_kernel(const u64* __restrict__ keys, int64_t n, int pass,
                                                               unsigned* __restrict__ state)
{
    __shared__ unsigned hist[256];
    hist[threadIdx.x] = 0u;
    __syncthreads();
    const int shift = 56 - 8 * pass;
    const u64 prefix = ((const u64*)(state + TK_STATE_WORDS))[0];
    int cur = -1;
    unsigned run = 0u;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const u64 key = keys[i];
        if (pass > 0 && (key >> (shift + 8)) != (prefix >> (shift + 8))) continue;
        const int d = (int)(key >> shift & 255ull);
        if (d != cur) {
            if (run) atomicAdd(&hist[cur], run);
            cur = d; run = 0u;
        }
        ++run;
    }
    if (run) atomicAdd(&hist[cur], run);
    __syncthreads();
    if (hist[threadIdx.x]) atomicAdd(&state[pass * 256 + threadIdx.x], hist[threadIdx.x]);
}

// the digit that holds the k_rem-th largest key of this pass: walk the histogram from the top
__global__ void topk_select_pick_kernel(int pass, unsigned* __restrict__ state)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    u64* s = (u64*)(state + TK_STATE_WORDS);
    const unsigned* h = state + pass * 256;
    u64 rem = s[1];
    int d = 255;
    for (; d > 0; --d) {
        if (rem <= (u64)h[d]) break;
        rem -= h[d];
    }
    s[0] |= (u64)d << (56 - 8 * pass);
    s[1] = rem;
}

__global__ __launch_bounds__(256) void topk_flags_kernel(const u64* __restrict__ keys, int64_t n, const unsigned* __restrict__ state,
                                                         int32_t* __restrict__ above, int32_t* __restrict__ ties)
{
    const u64 t = ((const u64*)(state + TK_STATE_WORDS))[0];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const u64 key = keys[i];
        above[i] = key > t;
        ties[i] = key == t;
    }
}

// survivors in index order: the keys above the threshold first, then the lowest-index ties.  The keys are stored
// inverted, so that the ascending sort that follows yields descending scores.
__global__ __launch_bounds__(256) void topk_compact_kernel(const u64* __restrict__ keys, int64_t n, const unsigned* __restrict__ state,
                                                           const int32_t* __restrict__ above, const int32_t* __restrict__ ties,
                                                           int64_t k, u64* __restrict__ out_keys, int32_t* __restrict__ out_idx)
{
    const u64* s = (const u64*)(state + TK_STATE_WORDS);
    const u64 t = s[0];
    const int64_t n_ties = (int64_t)s[1], n_above = k - n_ties;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const u64 key = keys[i];
        int64_t pos = -1;
        if (key > t) pos = above[i];
        else if (key == t && ties[i] < n_ties) pos = n_above + ties[i];
        if (pos >= 0 && pos < k) {
            out_keys[pos] = ~key;
            out_idx[pos] = (int32_t)i;
        }
    }
}

// One pass of the stable least-significant-digit sort of the survivors.  Single-wave workgroups, each over a contiguous
// chunk: counts[digit * nblocks + block] scanned exclusively is where the block's run of that digit begins.
__global__ __launch_bounds__(64) void topk_sort_hist_kernel(const u64* __restrict__ keys, int64_t k, int shift,
                                                            int32_t* __restrict__ counts)
{
    __shared__ int hist[256];
    for (int e = threadIdx.x; e < 256; e += 64) hist[e] = 0;
    __syncthreads();
    const int64_t beg = (int64_t)blockIdx.x * TK_SORT_CHUNK;
    const int64_t end = beg + TK_SORT_CHUNK < k ? beg + TK_SORT_CHUNK : k;
    for (int64_t i = beg + threadIdx.x; i < end; i += 64) atomicAdd(&hist[(int)(keys[i] >> shift & 255ull)], 1);
    __syncthreads();
    for (int e = threadIdx.x; e < 256; e += 64) counts[(int64_t)e * gridDim.x + blockIdx.x] = hist[e];
}

// Scatter of the same chunk, 64 consecutive items per round: a lane's rank among the lanes of the round that hold its
// digit comes from eight ballots, the digit's running offset lives in LDS and is advanced by the first lane of each group.
__global__ __launch_bounds__(64) void topk_sort_scatter_kernel(const u64* __restrict__ keys, const int32_t* __restrict__ idx, int64_t k,
                                                               int shift, const int32_t* __restrict__ offsets,
                                                               u64* __restrict__ out_keys, int32_t* __restrict__ out_idx,
                                                               int64_t* __restrict__ out_ids)
{
    __shared__ int off[256];
    for (int e = threadIdx.x; e < 256; e += 64) off[e] = offsets[(int64_t)e * gridDim.x + blockIdx.x];
    __syncthreads();
    const int lane = threadIdx.x;
    const int64_t beg = (int64_t)blockIdx.x * TK_SORT_CHUNK;
    const int64_t end = beg + TK_SORT_CHUNK < k ? beg + TK_SORT_CHUNK : k;
    for (int64_t base = beg; base < end; base += 64) {
        const int64_t i = base + lane;
        const bool valid = i < end;
        const u64 key = valid ? keys[i] : 0ull;
        const int32_t id = valid ? idx[i] : 0;
        const int d = (int)(key >> shift & 255ull);
        u64 same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const u64 set = __ballot(valid && (d >> b & 1));
            same &= (d >> b & 1) ? set : ~set;
        }
        const int rank = __popcll(same & ((1ull << lane) - 1ull));
        const int64_t pos = valid ? (int64_t)off[d] + rank : -1;
        __syncthreads();
        if (valid && rank == 0) off[d] += __popcll(same);
        __syncthreads();
        if (pos >= 0 && pos < k) {
            if (out_ids) out_ids[pos] = id;
            else { out_keys[pos] = key; out_idx[pos] = id; }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// spaced greedy selection
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SP_THREADS = 1024;          // the walk: one workgroup, one candidate per thread and chunk
constexpr int SP_WAVES = SP_THREADS / 64;
constexpr int SP_USED_TILE = 256;         // used coordinates staged in LDS per round of the blocking pass
constexpr int SP_NONE = 1 << 30;          // "no live lane" in a wave's slot

template <typename T>
__device__ __forceinline__ void sp_load(const void* coords, int64_t i, double& x, double& y, double& z)
{
    const T* p = (const T*)coords + 3 * i;
    x = (double)p[0]; y = (double)p[1]; z = (double)p[2];
}

// q blocks p: float64, every operation rounded on its own (-ffp-contract=off), strict
__device__ __forceinline__ bool sp_blocks(double px, double py, double pz, double qx, double qy, double qz, double s2)
{
    const double dx = px - qx, dy = py - qy, dz = pz - qz;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    return d2 < s2;
}

// dead[i] = candidate i lies within the spacing of a used point (or its id is outside [0, n) and is never dereferenced).
// One candidate per thread; the used coordinates stream through LDS in tiles and are read as broadcasts.
template <typename T>
__global__ __launch_bounds__(SP_USED_TILE) void spaced_used_kernel(const void* __restrict__ coords, int64_t n,
                                                                   const int64_t* __restrict__ cand, int64_t m,
                                                                   const int64_t* __restrict__ used, int64_t n_used, double s2,
                                                                   uint8_t* __restrict__ dead)
{
    __shared__ double ux[SP_USED_TILE], uy[SP_USED_TILE], uz[SP_USED_TILE];
    const int64_t chunks = (m + SP_USED_TILE - 1) / SP_USED_TILE;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t i = c * SP_USED_TILE + threadIdx.x;
        const int64_t id = i < m ? cand[i] : -1;
        const bool ok = id >= 0 && id < n;
        double px = 0.0, py = 0.0, pz = 0.0;
        if (ok) sp_load<T>(coords, id, px, py, pz);
        bool hit = false;
        for (int64_t t0 = 0; t0 < n_used; t0 += SP_USED_TILE) {
            const int64_t j = t0 + threadIdx.x;
            double x = 0.0, y = 0.0, z = 0.0;
            if (j < n_used) sp_load<T>(coords, used[j], x, y, z);          // the ids were range-checked on the host
            ux[threadIdx.x] = x; uy[threadIdx.x] = y; uz[threadIdx.x] = z;
            __syncthreads();
            const int cnt = (int)(n_used - t0 < SP_USED_TILE ? n_used - t0 : SP_USED_TILE);
            for (int e = 0; e < cnt; ++e) hit |= sp_blocks(px, py, pz, ux[e], uy[e], uz[e], s2);
            __syncthreads();
        }
        if (i < m) dead[i] = (uint8_t)(!ok || hit);
    }
}

// The walk.  state = { acceptances so far, candidates consumed }.  The accepted coordinates live in LDS (reloaded from
// ids when a walk is resumed).  Per chunk of SP_THREADS candidates: every thread tests its candidate against what was
// accepted before the chunk; then the chunk is resolved in order -- each wave posts its lowest live lane with its
// coordinates, one barrier, every thread reads the SP_WAVES slots (the first occupied one is the lowest live candidate
// of the workgroup), the winner is accepted and the other live lanes test against it.  The slots are double-buffered,
// so a round is one barrier; the round that finds no live lane ends the chunk.
template <typename T>
__global__ __launch_bounds__(SP_THREADS) void spaced_walk_kernel(const void* __restrict__ coords, int64_t n,
                                                                 const int64_t* __restrict__ cand, int64_t m,
                                                                 const uint8_t* __restrict__ dead, double s2, int64_t k,
                                                                 int64_t* __restrict__ ids, int64_t* __restrict__ state, int resume)
{
    __shared__ double ax[WS_AL_SPACED_MAX_K], ay[WS_AL_SPACED_MAX_K], az[WS_AL_SPACED_MAX_K];
    __shared__ double wx[2][SP_WAVES], wy[2][SP_WAVES], wz[2][SP_WAVES];
    __shared__ int wl[2][SP_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t acc = resume ? state[0] : 0, before = resume ? state[1] : 0;
    if (acc < 0) acc = 0;
    if (acc > k) acc = k;
    for (int64_t j = tid; j < acc; j += SP_THREADS) {
        const int64_t id = ids[j];
        double x = 0.0, y = 0.0, z = 0.0;
        if (id >= 0 && id < n) sp_load<T>(coords, id, x, y, z);
        ax[j] = x; ay[j] = y; az[j] = z;
    }
    __syncthreads();
    int64_t consumed = 0;
    int round = 0;
    for (int64_t base = 0; base < m && acc < k; base += SP_THREADS) {
        const int64_t i = base + tid;
        const int64_t id = i < m ? cand[i] : -1;
        bool live = id >= 0 && id < n;
        if (live && dead) live = dead[i] == 0;
        double px = 0.0, py = 0.0, pz = 0.0;
        if (live) sp_load<T>(coords, id, px, py, pz);
        if (__any(live)) {
            bool hit = false;
            for (int64_t j = 0; j < acc; ++j) hit |= sp_blocks(px, py, pz, ax[j], ay[j], az[j], s2);
            live = live && !hit;
        }
        int last = -1;
        for (;;) {
            const u64 b = __ballot(live);
            const int buf = round & 1;
            ++round;
            const int first = b ? __ffsll((long long)b) - 1 : 0;
            if (lane == first) {
                wl[buf][wave] = b ? tid : SP_NONE;
                wx[buf][wave] = px; wy[buf][wave] = py; wz[buf][wave] = pz;
            }
            __syncthreads();
            int win = SP_NONE, ww = 0;
#pragma unroll
            for (int w = SP_WAVES - 1; w >= 0; --w) {
                const int v = wl[buf][w];
                if (v != SP_NONE) { win = v; ww = w; }
            }
            if (win == SP_NONE) break;
            if (tid == win) {
                ax[acc] = px; ay[acc] = py; az[acc] = pz;
                ids[acc] = id;
                live = false;
            } else if (live && sp_blocks(px, py, pz, wx[buf][ww], wy[buf][ww], wz[buf][ww], s2)) {
                live = false;
            }
            ++acc;
            if (acc == k) { last = win; break; }
        }
        consumed = last >= 0 ? base + last + 1 : (base + SP_THREADS < m ? base + SP_THREADS : m);
    }
    if (tid == 0) {
        state[0] = acc;
        state[1] = before + consumed;
    }
}

inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

// the launches of a spaced selection, from its sizes alone: shared by the launcher and its reporter
struct SpacedPlan {
    int f64, used_pass, used_blocks, used_tiles, tail, resume;
    int64_t chunks, off_used, off_dead, total;
};

SpacedPlan spaced_plan(int32_t coords_f64, int64_t m, int64_t n_used, int32_t resume)
{
    SpacedPlan p;
    if (m < 0) m = 0;
    if (n_used < 0) n_used = 0;
    p.f64 = coords_f64 != 0;
    p.used_pass = n_used > 0 && m > 0;
    p.used_blocks = p.used_pass ? ws_grid(m, SP_USED_TILE) : 0;
    p.used_tiles = (int)ws_ceil_div(n_used, SP_USED_TILE);
    p.chunks = ws_ceil_div(m, SP_THREADS);
    p.tail = (int)(m % SP_THREADS);
    p.resume = resume != 0;
    p.off_used = 0;
    p.off_dead = align256(n_used * 8);
    p.total = p.off_dead + align256(m) + 256;
    return p;
}

struct TopkLayout {
    int64_t excluded, keys, above, ties, scan, state, keys_a, keys_b, idx_a, idx_b, counts, total;
    int sort_blocks;
};

TopkLayout topk_layout(int64_t n, int64_t k)
{
    TopkLayout l;
    if (n < 0) n = 0;
    if (k < 0) k = 0;
    l.sort_blocks = (int)(ws_ceil_div(k, TK_SORT_CHUNK) > 0 ? ws_ceil_div(k, TK_SORT_CHUNK) : 1);
    const int64_t n_counts = 256ll * l.sort_blocks;
    int64_t o = 0;
    l.excluded = o; o += align256(ws_ceil_div(n, 32) * 4 + 4);
    l.keys = o;     o += align256(n * 8);
    l.above = o;    o += align256((n + 1) * 4);
    l.ties = o;     o += align256((n + 1) * 4);
    l.scan = o;     o += align256(ws_scan_scratch_items(n > n_counts ? n : n_counts) * 4);
    l.state = o;    o += align256(TK_STATE_WORDS * 4 + 16);
    l.keys_a = o;   o += align256(k * 8);
    l.keys_b = o;   o += align256(k * 8);
    l.idx_a = o;    o += align256(k * 4);
    l.idx_b = o;    o += align256(k * 4);
    l.counts = o;   o += align256((n_counts + 1) * 4);
    l.total = o;
    return l;
}

}  // namespace

extern "C" {

int ws_al_point_scores(const float* probs, int64_t n, int32_t c, const double* class_score, float* entropy, int32_t* preds,
                       double* score, void* stream)
{
    WS_REQUIRE(n >= 0 && c >= 1, "bad sizes n=%lld c=%d", (long long)n, c);
    if (c > 32) return ws_fail(WS_ERR_UNSUPPORTED, "ws_al_point_scores: c=%d classes (at most 32)", c);
    if (n == 0) return WS_OK;
    WS_REQUIRE(probs && class_score && entropy && preds && score, "NULL argument");
    const int64_t tiles = ws_ceil_div(n, AL_ROWS);
    point_scores_kernel<<<ws_grid(tiles, 1), AL_ROWS, sizeof(float) * AL_ROWS * (c | 1), (hipStream_t)stream>>>(
        probs, n, c, class_score, entropy, preds, score);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_al_anchor_scores(const float* entropy, const int32_t* preds, int64_t n, const int64_t* anchor_ptr, const int64_t* anchor_idx,
                        int64_t nnz, int64_t n_anchors, const double* class_score, int32_t c, float* out, void* stream)
{
    WS_REQUIRE(n >= 0 && nnz >= 0 && n_anchors >= 0 && c >= 1, "bad sizes n=%lld nnz=%lld anchors=%lld c=%d", (long long)n,
               (long long)nnz, (long long)n_anchors, c);
    if (c > 32) return ws_fail(WS_ERR_UNSUPPORTED, "ws_al_anchor_scores: c=%d classes (at most 32)", c);
    if (n_anchors == 0) return WS_OK;
    WS_REQUIRE(anchor_ptr && class_score && out && (nnz == 0 || (entropy && preds && anchor_idx)), "NULL argument");
    anchor_scores_kernel<<<ws_grid(n_anchors, 4), 256, 0, (hipStream_t)stream>>>(entropy, preds, n, anchor_ptr, anchor_idx, nnz,
                                                                                n_anchors, class_score, c, out);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int64_t ws_topk_scratch_bytes(int64_t n, int64_t k) { return topk_layout(n, k).total; }

int ws_topk_select(const double* score, int64_t n, const int64_t* h_exclude, int64_t m, int64_t k, int64_t* ids, void* scratch,
                   void* stream)
{
    WS_REQUIRE(n >= 0 && m >= 0 && k >= 0 && n <= (1ll << 30), "bad sizes n=%lld m=%lld k=%lld", (long long)n, (long long)m,
               (long long)k);
    WS_REQUIRE(m == 0 || h_exclude, "NULL argument");
    // the used ids as a bitmap (host): range check, duplicates collapse, and the device cost no longer depends on m
    std::vector<unsigned> bits((size_t)ws_ceil_div(n, 32) + 1, 0u);
    int64_t unique = 0;
    for (int64_t e = 0; e < m; ++e) {
        const int64_t id = h_exclude[e];
        WS_REQUIRE(id >= 0 && id < n, "exclude[%lld] = %lld outside [0, %lld)", (long long)e, (long long)id, (long long)n);
        unsigned& w = bits[(size_t)(id >> 5)];
        const unsigned b = 1u << (id & 31);
        unique += !(w & b);
        w |= b;
    }
    WS_REQUIRE(k <= n - unique, "k=%lld but only %lld of n=%lld ids are not excluded", (long long)k, (long long)(n - unique),
               (long long)n);
    if (k == 0) return WS_OK;
    WS_REQUIRE(score && ids && scratch, "NULL argument");

    hipStream_t st = (hipStream_t)stream;
    const TopkLayout l = topk_layout(n, k);
    char* base = (char*)scratch;
    unsigned* excluded = (unsigned*)(base + l.excluded);
    u64* keys = (u64*)(base + l.keys);
    int32_t* above = (int32_t*)(base + l.above);
    int32_t* ties = (int32_t*)(base + l.ties);
    int32_t* scan = (int32_t*)(base + l.scan);
    unsigned* state = (unsigned*)(base + l.state);
    u64* keys_ab[2] = {(u64*)(base + l.keys_a), (u64*)(base + l.keys_b)};
    int32_t* idx_ab[2] = {(int32_t*)(base + l.idx_a), (int32_t*)(base + l.idx_b)};
    int32_t* counts = (int32_t*)(base + l.counts);

    // pageable source: the runtime returns once the copy has left `bits`, which on ROCm means after the work queued on
    // `stream` before it -- the one host wait of this entry (weasal_hip.h); no result is read back
    WS_HIP(hipMemcpyAsync(excluded, bits.data(), bits.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
    topk_init_kernel<<<1, 256, 0, st>>>(state, (long long)k);
    WS_LAUNCH_CHECK();
    const int grid = ws_grid(n, 256 * 8, 2048);
    topk_keys_kernel<<<grid, 256, 0, st>>>(score, n, excluded, keys);
    WS_LAUNCH_CHECK();
    for (int pass = 0; pass < 8; ++pass) {
        topk_select_hist_kernel<<<grid, 256, 0, st>>>(keys, n, pass, state);
        WS_LAUNCH_CHECK();
        topk_select_pick_kernel<<<1, 64, 0, st>>>(pass, state);
        WS_LAUNCH_CHECK();
    }
    topk_flags_kernel<<<grid, 256, 0, st>>>(keys, n, state, above, ties);
    WS_LAUNCH_CHECK();
    int rc = ws_exclusive_scan_i32(above, above, n, scan, st);
    if (rc) return rc;
    rc = ws_exclusive_scan_i32(ties, ties, n, scan, st);
    if (rc) return rc;
    topk_compact_kernel<<<grid, 256, 0, st>>>(keys, n, state, above, ties, k, keys_ab[0], idx_ab[0]);
    WS_LAUNCH_CHECK();
    const int nb = l.sort_blocks;
    for (int pass = 0; pass < 8; ++pass) {
        const int src = pass & 1, dst = src ^ 1;
        topk_sort_hist_kernel<<<nb, 64, 0, st>>>(keys_ab[src], k, 8 * pass, counts);
        WS_LAUNCH_CHECK();
        rc = ws_exclusive_scan_i32(counts, counts, 256ll * nb, scan, st);
        if (rc) return rc;
        topk_sort_scatter_kernel<<<nb, 64, 0, st>>>(keys_ab[src], idx_ab[src], k, 8 * pass, counts, keys_ab[dst], idx_ab[dst],
                                                    pass == 7 ? ids : nullptr);
        WS_LAUNCH_CHECK();
    }
    return WS_OK;
}

int64_t ws_al_spaced_scratch_bytes(int64_t m, int64_t n_used, int64_t k)
{
    (void)k;                                   // the accepted coordinates live in LDS
    return spaced_plan(0, m, n_used, 0).total;
}

// sizes and the spacing: what both the launcher and its reporter refuse, nothing of it on the device
static int spaced_check(int64_t n, int64_t m, int64_t n_used, double spacing, int64_t k)
{
    WS_REQUIRE(spacing > 0.0 && spacing < __builtin_inf(), "spacing=%g: a finite spacing above 0 is required", spacing);
    WS_REQUIRE(n >= 0 && m >= 0 && n_used >= 0 && k >= 0, "bad sizes n=%lld m=%lld n_used=%lld k=%lld", (long long)n, (long long)m,
               (long long)n_used, (long long)k);
    if (k > WS_AL_SPACED_MAX_K)
        return ws_fail(WS_ERR_UNSUPPORTED, "ws_al_spaced_select: k=%lld (at most WS_AL_SPACED_MAX_K = %d: the accepted coordinates "
                       "are resident in LDS)", (long long)k, WS_AL_SPACED_MAX_K);
    return WS_OK;
}

int ws_al_spaced_select(const void* coords, int32_t coords_f64, int64_t n, const int64_t* cand, int64_t m, const int64_t* h_used,
                        int64_t n_used, double spacing, int64_t k, int64_t* ids, int64_t* state, int32_t resume, void* scratch,
                        void* stream)
{
    if (int rc = spaced_check(n, m, n_used, spacing, k)) return rc;
    WS_REQUIRE(n_used == 0 || h_used, "NULL argument");
    for (int64_t e = 0; e < n_used; ++e)
        WS_REQUIRE(h_used[e] >= 0 && h_used[e] < n, "used[%lld] = %lld outside [0, %lld)", (long long)e, (long long)h_used[e],
                   (long long)n);
    hipStream_t st = (hipStream_t)stream;
    if (k == 0 || m == 0) {
        if (!resume && state) WS_HIP(hipMemsetAsync(state, 0, 2 * sizeof(int64_t), st));
        return WS_OK;
    }
    WS_REQUIRE(coords && cand && ids && state && scratch, "NULL argument");
    const SpacedPlan p = spaced_plan(coords_f64, m, n_used, resume);
    const double s2 = spacing * spacing;
    int64_t* used = (int64_t*)((char*)scratch + p.off_used);
    uint8_t* dead = p.used_pass ? (uint8_t*)scratch + p.off_dead : nullptr;
    if (p.used_pass) {
        // pageable source, as in ws_topk_select: the copy has left h_used when the call returns
        WS_HIP(hipMemcpyAsync(used, h_used, (size_t)n_used * sizeof(int64_t), hipMemcpyHostToDevice, st));
        if (p.f64) spaced_used_kernel<double><<<p.used_blocks, SP_USED_TILE, 0, st>>>(coords, n, cand, m, used, n_used, s2, dead);
        else spaced_used_kernel<float><<<p.used_blocks, SP_USED_TILE, 0, st>>>(coords, n, cand, m, used, n_used, s2, dead);
        WS_LAUNCH_CHECK();
    }
    if (p.f64) spaced_walk_kernel<double><<<1, SP_THREADS, 0, st>>>(coords, n, cand, m, dead, s2, k, ids, state, resume != 0);
    else spaced_walk_kernel<float><<<1, SP_THREADS, 0, st>>>(coords, n, cand, m, dead, s2, k, ids, state, resume != 0);
    WS_LAUNCH_CHECK();
    return WS_OK;
}

int ws_al_spaced_variant(int32_t coords_f64, int64_t n, int64_t m, int64_t n_used, double spacing, int64_t k, int32_t resume,
                         char* text, int32_t cap)
{
    WS_REQUIRE(text && cap > 0, "bad argument");
    if (int rc = spaced_check(n, m, n_used, spacing, k)) return rc;
    if (k == 0 || m == 0) {
        snprintf(text, (size_t)cap, "none (%s)%s", k == 0 ? "k == 0" : "m == 0", resume ? "" : " state zeroed");
        return WS_OK;
    }
    const SpacedPlan p = spaced_plan(coords_f64, m, n_used, resume);
    char used[96] = "no used pass";
    if (p.used_pass)
        snprintf(used, sizeof used, "spaced_used_kernel<%s> blocks=%d tiles=%d", p.f64 ? "double" : "float", p.used_blocks, p.used_tiles);
    snprintf(text, (size_t)cap, "%s + spaced_walk_kernel<%s> chunks=%lld tail=%d resume=%d", used, p.f64 ? "double" : "float",
             (long long)p.chunks, p.tail, p.resume);
    return WS_OK;
}

}  // extern "C"
