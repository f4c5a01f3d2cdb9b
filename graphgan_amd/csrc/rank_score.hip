// rank_score.hip -- full-ranking link evaluation: for each query (u, v) the exact position of column v in row u of
// S = E . E^T (no bias) among ALL candidate columns, in the order of gg_topk_scores (score descending, column ascending, -0
// counting as +0), optionally without u itself and u's neighbours in the resident training graph.  The third consumer of the
// tile stream (score_tiles.h) and the cheapest per tile: a query is one requested row of the stream, and every score of that
// row is compared with ONE threshold -- the target's own score and column -- and counted.  Nothing of size m x N exists at
// any time.
//
// "c is ahead of v" is key(s(u, c), c) > key(s(u, v), v) with topk_score.hip's key = ord(score) << 32 | ~col; on finite
// scores that is
//     s(u, c) > s(u, v)  ||  (s(u, c) == s(u, v)  &&  c < v)
// in fp32 compares (-0 == +0 there as in ord), which is what the kernels evaluate.  The target column never counts itself.
//
// Per pass of 4 096 queries, two kernels:
//   rank_gather_kernel   one wavefront per query scores the GATHERED columns [v, u, sorted adj(u) ...] with the stream's own
//                        arithmetic: the first gives the threshold (= score_out), the others -- each distinct excluded column
//                        once, v itself never -- give n_cand and the number of excluded columns ahead of the target, which
//                        starts the query's rank at 1 - that number (exclude = 0: only [v], rank starts at 1);
//   rank_f32_kernel /    the stream counts, UNFILTERED, the columns ahead of the target -- per lane 16 integer counters beside
//   rank_bf16_kernel     the 16 thresholds of the rows it holds -- folds them over the 32 lanes of each half-wave and the 4
//                        wavefronts at the end of the workgroup's column split and adds one integer per (split, row) to the
//                        query's rank (integer atomics: the sum does not depend on their order).
// An exclusion test per counted column in the stream (as the top-K consumer does for its rare candidates) would be a binary
// search for half the columns of a poorly ranked target.
// The gathered scores must be the stream's bits:
//   fp32: the k-ordered fmaf chain from 0.0 over the padded row (v_mfma_f32_32x32x2_f32 is that chain);
//   bf16: the same v_mfma_f32_32x32x16_bf16 sequence over the same bf16_piece fragments from a zero accumulator -- the
//         instruction's internal summation order is no scalar chain -- with the gathered nodes as the B operand (32 per
//         tile) and u as every row of the A operand.
#include <math.h>

#include <algorithm>

#include "score_tiles.h"

namespace gg {

namespace {

constexpr int RK_CHUNK = 4096;  // queries per internal pass

// c (score x) ahead of the target (score t, column v)?
__device__ __forceinline__ bool ahead_of(float x, int c, float t, int v) { return x > t || (x == t && c < v); }

struct RankArgs {
    const int32_t *u, *v;     // [n] the pass's queries: row node, target column
    int n;
    const int64_t *adj_ptr;   // exclusion: the graph's row offsets and its column lists sorted per node (NULL: exclude = 0)
    const int32_t *adj;
    float *score;             // [n] s(u, v): written by the gather kernel, the stream's threshold
    int32_t *n_cand;          // [n]
    int32_t *rank;            // [n] 1 - (excluded columns ahead) from the gather kernel; the stream adds its counts
};

// Score of (u, c) for the lane's gathered column: KS = 0 fp32 on E, else bf16 on the tiled copy Eb (a tile of 32 columns per
// wavefront: lanes l and l ^ 32 hold the two k-halves of column l & 31 and both get its score).  Wavefront-uniform control flow.
template <int KS>
__device__ __forceinline__ float gathered_score(const float *E, int ld, const uint4 *Eb, int u, int c) {
    if constexpr (KS == 0) {
        const float *a = E + (int64_t)u * ld, *b = E + (int64_t)c * ld;
        float acc = 0.f;
        for (int k = 0; k < ld; k += 4) {
            const float4 x = *(const float4 *)(a + k), y = *(const float4 *)(b + k);
            acc = __builtin_fmaf(x.x, y.x, acc);
            acc = __builtin_fmaf(x.y, y.y, acc);
            acc = __builtin_fmaf(x.z, y.z, acc);
            acc = __builtin_fmaf(x.w, y.w, acc);
        }
        return acc;
    } else {
        const int half = (threadIdx.x & 63) >> 5;
        union Frag { uint4 q; bf16x8 v; };
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            Frag fa, fb;
            fa.q = Eb[bf16_piece(u, s, half, KS)];
            fb.q = Eb[bf16_piece(c, s, half, KS)];
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa.v, fb.v, acc, 0, 0, 0);
        }
        return acc[0];  // (every row of the tile is u)
    }
}

// One wavefront per query.  Entries: 0 = v (the threshold), and with the exclusion 1 = u, 2 .. = the sorted adjacency of u.
template <int KS>
__global__ __launch_bounds__(256) void rank_gather_kernel(const float *E, int ld, const uint4 *Eb, int n_node, RankArgs o) {
    constexpr int EPI = KS == 0 ? 64 : 32;  // entries per iteration
    const int lane = threadIdx.x & 63;
    const int q = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (q >= o.n) return;
    const int u = __builtin_amdgcn_readfirstlane(o.u[q]), v = __builtin_amdgcn_readfirstlane(o.v[q]);
    int64_t b = 0;
    int n_ent = 1;
    if (o.adj) {
        b = o.adj_ptr[u];
        n_ent = __builtin_amdgcn_readfirstlane(2 + (int)(o.adj_ptr[u + 1] - b));
    }
    const int slot = KS == 0 ? lane : (lane & 31);
    float t = 0.f;
    int n_excl = 0, n_ahead = 0;  // distinct excluded columns other than v; those of them ahead of v
    for (int e0 = 0; e0 < n_ent; e0 += EPI) {
        const int e = e0 + slot;
        int c = v;
        bool live = false;  // an excluded column, counted once, not v
        if (e == 1 && e < n_ent) {
            c = u;
            live = u != v;
        } else if (e >= 2 && e < n_ent) {
            const int64_t p = b + e - 2;
            c = o.adj[p];
            live = c != v && c != u && !(e > 2 && o.adj[p - 1] == c);
        }
        const float x = gathered_score<KS>(E, ld, Eb, u, c);
        if (e0 == 0) t = __shfl(x, 0, 64);
        if (KS != 0) live = live && lane < 32;
        n_excl += __builtin_popcountll(__builtin_amdgcn_ballot_w64(live));
        n_ahead += __builtin_popcountll(__builtin_amdgcn_ballot_w64(live && ahead_of(x, c, t, v)));
    }
    if (lane == 0) {
        o.score[q] = t;
        o.n_cand[q] = n_node - n_excl;
        o.rank[q] = 1 - n_ahead;
    }
}

// The consumer handed to the producers of score_tiles.h: per lane the thresholds (score, column) of the 16 rows it holds
// (tile_row(reg, lane >> 5), the matrix instruction's C layout) and 16 integer counters.
struct CountConsumer {
    float t[16];
    int tcol[16], cnt[16];
    const RankArgs &o;
    const int r0;
    __device__ __forceinline__ CountConsumer(const RankArgs &o_, int r0_) : o(o_), r0(r0_) {}
    __device__ __forceinline__ void init() {
        const int half = (threadIdx.x & 63) >> 5;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = r0 + tile_row(reg, half);
            t[reg] = row < o.n ? o.score[row] : INFINITY;  // (rows behind the pass count nothing)
            tcol[reg] = row < o.n ? o.v[row] : -1;
            cnt[reg] = 0;
        }
    }
    __device__ __forceinline__ float start(int, bool) const { return 0.f; }
    __device__ __forceinline__ void operator()(const f32x16 &acc, int col, bool ok) {
        if (ok) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) cnt[reg] += ahead_of(acc[reg], col, t[reg], tcol[reg]) ? 1 : 0;
        }
    }
    __device__ __forceinline__ void operator()(const f32x16 (&acc)[1], int col, bool ok) { (*this)(acc[0], col, ok); }
    // End of the workgroup's column split: the counters summed over the 32 lanes of each half-wave (lanes l and l ^ 32 hold
    // different rows) and the 4 wavefronts, one integer per row added to the query's rank.
    __device__ __forceinline__ void finish(int (*sh)[32]) {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            int c = cnt[reg];
#pragma unroll
            for (int off = 16; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
            if ((lane & 31) == 0) sh[wv][tile_row(reg, lane >> 5)] = c;
        }
        __syncthreads();
        const int tr = threadIdx.x;
        if (tr < 32 && r0 + tr < o.n) {
            const int c = sh[0][tr] + sh[1][tr] + sh[2][tr] + sh[3][tr];
            if (c) atomicAdd(o.rank + r0 + tr, c);
        }
    }
};

// Launch shapes of topk_f32_kernel / topk_bf16_kernel: grid = (column splits, 32-row tiles), 4 wavefronts of 32 columns each.
__global__ __launch_bounds__(256) void rank_f32_kernel(const float *E, int n_node, int ld, int cols_per_split, RankArgs o) {
    extern __shared__ float As_all[];  // [32][ld + 1]: the tile's 32 requested rows, staged once
    __shared__ float Bs[128][ST_KC + 1];
    __shared__ int sh_cnt[4][32];
    const int split = blockIdx.x, r0 = blockIdx.y * 32;
    const int cbeg = split * cols_per_split, cend = min(n_node, cbeg + cols_per_split);
    CountConsumer count(o, r0);
    f32_score_tiles(E, ld, o.u, o.n, r0, cbeg, cend, As_all, Bs, count);
    count.finish(sh_cnt);
}

template <int KS>
__global__ __launch_bounds__(256) void rank_bf16_kernel(const uint4 *Eb, int n_node, int cols_per_split, RankArgs o) {
    __shared__ int sh_cnt[4][32];
    const int split = blockIdx.x, r0 = blockIdx.y * 32;
    const int cbeg = split * cols_per_split, cend = min(n_node, cbeg + cols_per_split);
    CountConsumer count(o, r0);
    bf16_score_tiles<KS, 1, (KS <= 16)>(Eb, o.u, o.n, r0, cbeg, cend, count);
    count.finish(sh_cnt);
}

// first id outside [0, n_node), or -1
int64_t first_bad_id(const int32_t *ids, int64_t m, int n_node) {
    for (int64_t i = 0; i < m; ++i)
        if (ids[i] < 0 || ids[i] >= n_node) return i;
    return -1;
}

}  // namespace

}  // namespace gg

using namespace gg;

// gg_rank_scores: see include/graphgan_hip.h.
extern "C" int gg_rank_scores(gg_ctx *ctx, int32_t which, const int32_t *u, const int32_t *v, int64_t m, int32_t precision, int32_t exclude,
                              int32_t *rank_out, int32_t *n_cand_out, float *score_out, double *kernel_ms_out) {
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    GG_CHECK(ctx, which == 0 || which == 1, GG_EINVAL, "gg_rank_scores: which must be 0 (generator) or 1 (discriminator)");
    GG_CHECK(ctx, precision == 0 || precision == 1, GG_EINVAL, "gg_rank_scores: precision must be 0 (fp32) or 1 (bf16)");
    GG_CHECK(ctx, exclude == 0 || exclude == 1, GG_EINVAL, "gg_rank_scores: exclude must be 0 or 1");
    GG_CHECK(ctx, u && v && rank_out, GG_EINVAL, "gg_rank_scores: bad argument");
    GG_CHECK(ctx, m >= 1 && m <= 0x7fffffffLL, GG_EINVAL, "gg_rank_scores: m = %lld outside [1, 2^31 - 1]", (long long)m);
    GG_CHECK(ctx, !exclude || ctx->g_rowptr, GG_EINVAL, "gg_rank_scores: exclude = 1 needs the training graph (gg_set_graph_csr)");
    const int n = ctx->n_node, ld = ctx->ld;
    GG_CHECK(ctx, precision == 0 || ctx->n_emb <= 512, GG_EINVAL, "gg_rank_scores: bf16 supports n_emb <= 512 (got %d)", ctx->n_emb);
    const size_t dyn = sizeof(float) * 32 * (size_t)(ld + 1);
    GG_CHECK(ctx, precision == 1 || dyn <= 140 * 1024, GG_EINVAL, "gg_rank_scores: fp32 supports n_emb <= 1116 (got %d)", ctx->n_emb);
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    int64_t bad = first_bad_id(u, m, n);
    GG_CHECK(ctx, bad < 0, GG_EINVAL, "gg_rank_scores: u[%lld] = %d out of range [0, %d)", (long long)bad, u[bad], n);
    bad = first_bad_id(v, m, n);
    GG_CHECK(ctx, bad < 0, GG_EINVAL, "gg_rank_scores: v[%lld] = %d out of range [0, %d)", (long long)bad, v[bad], n);
    GG_HIP(ctx, hipSetDevice(ctx->device));
    if (exclude) {
        const int rc = ensure_sorted_adjacency(ctx);
        if (rc != GG_OK) return rc;
    }
    const Bf16Shape bs = bf16_shape(ctx->n_emb);
    const int chunk = (int)std::min<int64_t>(m, RK_CHUNK);
    const ColumnSplit cs = column_split(n, cdiv(chunk, 32), 2048);  // column splits as K7's and the top-K stream's
    const Model &M = ctx->model[which];
    DevBuf d_u, d_v, d_score, d_cand, d_rank, d_bf;
    auto rel = [&]() { d_u.release(); d_v.release(); d_score.release(); d_cand.release(); d_rank.release(); d_bf.release(); };
    hipError_t e = d_u.reserve(sizeof(int32_t) * chunk);
    if (e == hipSuccess) e = d_v.reserve(sizeof(int32_t) * chunk);
    if (e == hipSuccess) e = d_score.reserve(sizeof(float) * chunk);
    if (e == hipSuccess) e = d_cand.reserve(sizeof(int32_t) * chunk);
    if (e == hipSuccess) e = d_rank.reserve(sizeof(int32_t) * chunk);
    if (e == hipSuccess && precision == 1) e = bf16_table(ctx, which, bs.ld16, d_bf);
    if (e != hipSuccess) { rel(); return fail(ctx, GG_ENOMEM, "gg_rank_scores: %s", hipGetErrorString(e)); }
    if (precision == 0 && dyn > 48 * 1024) (void)hipFuncSetAttribute((const void *)rank_f32_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    const uint4 *Eb = (const uint4 *)d_bf.p;
    double ms_total = 0.0;
    for (int64_t c0 = 0; c0 < m && e == hipSuccess; c0 += chunk) {
        const int cr = (int)std::min<int64_t>(chunk, m - c0);
        e = hipMemcpyAsync(d_u.p, u + c0, sizeof(int32_t) * cr, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_v.p, v + c0, sizeof(int32_t) * cr, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) break;
        RankArgs o{d_u.as<int32_t>(), d_v.as<int32_t>(), cr, exclude ? ctx->g_rowptr : nullptr, exclude ? ctx->topk_adj.as<int32_t>() : nullptr,
                   d_score.as<float>(), d_cand.as<int32_t>(), d_rank.as<int32_t>()};
        const dim3 ggrid(cdiv(cr, 4)), grid(cs.splits, cdiv(cr, 32));
        (void)hipEventRecord(ctx->ev0, ctx->stream);
        if (precision == 0) {
            hipLaunchKernelGGL(rank_gather_kernel<0>, ggrid, dim3(256), 0, ctx->stream, M.E, ld, Eb, n, o);
            hipLaunchKernelGGL(rank_f32_kernel, grid, dim3(256), dyn, ctx->stream, M.E, n, ld, cs.cols_per_split, o);
        } else {
#define GG_RANK_BF16(KSV)                                                                                         \
    do {                                                                                                          \
        hipLaunchKernelGGL(rank_gather_kernel<KSV>, ggrid, dim3(256), 0, ctx->stream, M.E, ld, Eb, n, o);         \
        hipLaunchKernelGGL(rank_bf16_kernel<KSV>, grid, dim3(256), 0, ctx->stream, Eb, n, cs.cols_per_split, o);  \
    } while (0)
            if (bs.KS == 4) GG_RANK_BF16(4);
            else if (bs.KS == 8) GG_RANK_BF16(8);
            else if (bs.KS == 16) GG_RANK_BF16(16);
            else GG_RANK_BF16(32);
#undef GG_RANK_BF16
        }
        (void)hipEventRecord(ctx->ev1, ctx->stream);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(rank_out + c0, d_rank.p, sizeof(int32_t) * cr, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && n_cand_out) e = hipMemcpyAsync(n_cand_out + c0, d_cand.p, sizeof(int32_t) * cr, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && score_out) e = hipMemcpyAsync(score_out + c0, d_score.p, sizeof(float) * cr, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        float ms = 0.f;
        if (e == hipSuccess) (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
        ms_total += ms;
    }
    rel();
    if (e != hipSuccess) return fail(ctx, GG_EHIP, "gg_rank_scores: %s", hipGetErrorString(e));
    if (kernel_ms_out) *kernel_ms_out = ms_total;
    return GG_OK;
}
