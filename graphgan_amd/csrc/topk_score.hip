// topk_score.hip -- streamed top-K node retrieval: for each requested node u the k best columns of S[u, :] = E[u] . E^T
// (no bias: the evaluator's score, link_prediction.py:26-27), optionally without u itself and u's neighbours in the resident
// training graph.  The rows of S are produced tile by tile on the matrix cores exactly as K7 (all_score.hip) produces them and
// consumed in registers; nothing of size n_rows x N exists at any time.
//
// Order of a result row: score descending, column ascending.  Both are packed into ONE 64-bit key,
//     key = ord(score) << 32 | ~col        (ord: the monotone unsigned image of an fp32; -0 counts as +0)
// so "better" is "larger key", every key is distinct (columns are), and 0 is below every real key: an empty list slot.
//
// Work split: grid = (column splits, 32-row tiles); a workgroup's 4 wavefronts take 32 columns each of every 128-column tile
// of its split.  Every WAVEFRONT keeps, for each of the tile's 32 rows, a private sorted K-list (in the partial buffer in
// global memory -- it is touched only when it changes) and the list's K-th score tau in registers.  Per tile and lane the
// 16 scores it holds are compared with their rows' tau and OR-ed into one flag; one ballot per tile decides, uniformly for the
// wavefront, whether anything can enter a list.  After the first few tiles tau is high and nearly every tile costs those
// 16 compares; the rare tiles with candidates take the insertion path: per (row, half-wave) the candidates are checked for
// eligibility (exclude: a binary search in the sorted adjacency of the row's node -- only scores >= tau ever get there, and an
// excluded column never enters a list, so it cannot raise tau), ranked among themselves and against the list, and merged
// in place; the new K-th key becomes the row's tau.  A wavefront's columns only grow, so a candidate never ties a list entry.
// topk_merge_kernel then merges the (split, wavefront) lists of a row on the device (one workgroup per row, rank merge in LDS,
// a list whose head does not beat the running K-th key is skipped).
// gg_topk_metric (cosine / squared Euclidean order, a candidate set, exclude = 2) runs the same kernels as further template
// instances: see ListConsumer.
// The tiles come from the producers K7's streamed consumer uses (score_tiles.h):
//   fp32: f32_score_tiles -- the k-ordered fmaf chain from 0.0, so the scores are bit-identical to gg_all_score (zero bias)
//         and the oracle's rows;
//   bf16: bf16_score_tiles on the tiled bf16 copy of the table (round to nearest even), fp32 accumulate from 0.0; the next
//         tile is prefetched while its fragments fit (KS <= 16).
#include <math.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "score_tiles.h"

namespace gg {

namespace {

typedef unsigned long long u64;

constexpr int TK_CHUNK = 4096;     // requested rows per internal pass
constexpr int TK_MAX_K = 256;
constexpr size_t TK_PART_CAP = size_t(256) << 20;  // bytes of partial lists per pass, at most

struct TopkOut {
    const int32_t *rows;      // [n_rows] node ids of the pass
    int n_rows, k;
    const int64_t *adj_ptr;   // exclusion: the graph's row offsets and its column lists sorted per node (NULL: exclude = 0)
    const int32_t *adj;
    u64 *part;                // [n_rows][n_sub][k] keys, descending, 0 = empty
    int n_sub;                // 4 per column split
    // gg_topk_metric only (the instances of gg_topk_scores read none of these):
    const float *colv;        // [n_node] the column's scalar: w_c = 1 / sqrt(h_c) (cosine), h_c = |x_c|^2 (l2)
    const uint32_t *member;   // [ceil(n_node / 32)] bit c: column c is a candidate (instances with a bitmap)
    int not_self;             // exclude = 2: column u is not eligible in row u (instances with a bitmap)
};

// The ordering value t of a score s under the metric (include/graphgan_hip.h, gg_topk_metric): one fp32 operation with the
// column's scalar.  Lists, tau and keys hold t; topk_merge_kernel maps t to the reported value with the row's scalar.
enum { TK_DOT = 0, TK_COS = 1, TK_L2 = 2 };

__device__ __forceinline__ u64 topk_key(float x, int col) {
    uint32_t u = __float_as_uint(x);
    u = u == 0x80000000u ? 0u : u;
    const uint32_t o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((u64)o << 32) | (uint32_t)~(uint32_t)col;
}

__device__ __forceinline__ float key_score(u64 key) {
    const uint32_t o = (uint32_t)(key >> 32);
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__device__ __forceinline__ u64 readlane64(u64 v, int j) {
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, j), hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), j);
    return ((u64)hi << 32) | lo;
}

// Merge the candidates of one row (lanes with `cand`, key `key`; all their columns lie behind every entry of the list) into
// the wavefront's list L (k keys, descending, zeros behind the last entry).  Wavefront-wide; returns the new k-th key (0: the
// list is not full).  Every lane reads what it needs before any lane writes (the loaded values feed the stores).
__device__ u64 wave_insert(u64 *L, int k, bool cand, u64 key) {
    const int lane = threadIdx.x & 63;
    const u64 m = __builtin_amdgcn_ballot_w64(cand);
    int pos = k;
    if (cand) {  // entries of L above the key: a prefix
        int lo = 0, hi = k;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (L[mid] > key) lo = mid + 1;
            else hi = mid;
        }
        pos = lo;
    }
    u64 lv[TK_MAX_K / 64];
    int sh[TK_MAX_K / 64];
#pragma unroll
    for (int q = 0; q < TK_MAX_K / 64; ++q) {
        const int i = lane + 64 * q;
        lv[q] = i < k ? L[i] : 0ull;
        sh[q] = 0;
    }
    u64 mm = m;
    while (mm) {  // (uniform: at most 32 candidates)
        const int j = __builtin_ctzll(mm);
        mm &= mm - 1;
        const u64 kj = readlane64(key, j);
        pos += (cand && kj > key) ? 1 : 0;
#pragma unroll
        for (int q = 0; q < TK_MAX_K / 64; ++q) sh[q] += kj > lv[q] ? 1 : 0;
    }
    u64 at_last = 0, old_last = 0;  // the key that lands at position k - 1; the one there before
#pragma unroll
    for (int q = 0; q < TK_MAX_K / 64; ++q) old_last = lane + 64 * q == k - 1 ? lv[q] : old_last;
#pragma unroll
    for (int q = 0; q < TK_MAX_K / 64; ++q) {
        const int i = lane + 64 * q, p = i + sh[q];
        if (i < k && lv[q] != 0 && p < k) {
            L[p] = lv[q];
            if (p == k - 1) at_last = lv[q];
        }
    }
    if (cand && pos < k) {
        L[pos] = key;
        if (pos == k - 1) at_last = key;
    }
    __threadfence_block();  // (the next insertion into this list reads what the lanes wrote)
    const u64 w = __builtin_amdgcn_ballot_w64(at_last != 0);
    return w ? readlane64(at_last, __builtin_ctzll(w)) : readlane64(old_last, (k - 1) & 63);  // (nothing entered: unchanged)
}

__device__ __forceinline__ bool adj_contains(const int32_t *a, int64_t n, int col) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < col) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && a[lo] == col;
}

// Per wavefront: the k-lists of the tile's 32 rows (sub-list `sub`) and, per lane, tau of the 16 rows it holds
// (tile_row(reg, lane >> 5), the matrix instruction's C layout).
struct WaveLists {
    float tau[16];
};

__device__ __forceinline__ u64 *list_of(const TopkOut &o, int row, int sub) { return o.part + ((int64_t)row * o.n_sub + sub) * o.k; }

__device__ __forceinline__ void lists_init(WaveLists &st, const TopkOut &o, int r0, int sub) {
    const int lane = threadIdx.x & 63, hi = lane >> 5;
    for (int rr = 0; rr < 32; ++rr) {
        if (r0 + rr >= o.n_rows) break;
        u64 *L = list_of(o, r0 + rr, sub);
        for (int i = lane; i < o.k; i += 64) L[i] = 0ull;
    }
    __threadfence_block();
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int row = r0 + tile_row(reg, hi);
        st.tau[reg] = row < o.n_rows ? -INFINITY : INFINITY;  // (rows behind the pass never take a candidate)
    }
}

// One finished 32 x 32 tile of the wavefront: lane holds column `col` (valid iff ok) of 16 rows; acc holds the ordering values.
// CAND: the membership bit of the column (and exclude = 2's "not the row's own node") is tested where the adjacency is: on the
// insertion path only, so an ineligible column never enters a list and never raises tau.
template <bool CAND>
__device__ __forceinline__ void lists_consume(WaveLists &st, const TopkOut &o, int r0, int sub, const f32x16 &acc, int col, bool ok) {
    bool any = false;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) any |= acc[reg] >= st.tau[reg];
    any &= ok;
    if (!__builtin_amdgcn_ballot_w64(any)) return;
    const int lane = threadIdx.x & 63, hi = lane >> 5;
#pragma unroll 1
    for (int reg = 0; reg < 16; ++reg) {
        float x = acc[0], t = st.tau[0];
#pragma unroll
        for (int r2 = 1; r2 < 16; ++r2) {
            x = reg == r2 ? acc[r2] : x;
            t = reg == r2 ? st.tau[r2] : t;
        }
        const bool p = ok && x >= t;
        const u64 pm = __builtin_amdgcn_ballot_w64(p);
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            if (((pm >> (32 * h)) & 0xffffffffull) == 0) continue;
            const int row = r0 + tile_row(reg, h);
            bool cand = p && hi == h;
            if (CAND && cand) cand = ((o.member[col >> 5] >> (col & 31)) & 1u) != 0 && !(o.not_self && col == o.rows[row]);
            if (cand && o.adj) {
                const int u = o.rows[row];
                const int64_t b = o.adj_ptr[u], e = o.adj_ptr[u + 1];
                cand = col != u && !adj_contains(o.adj + b, e - b, col);
            }
            const u64 kth = wave_insert(list_of(o, row, sub), o.k, cand, cand ? topk_key(x, col) : 0ull);
            const float nt = kth ? key_score(kth) : -INFINITY;
#pragma unroll
            for (int r2 = 0; r2 < 16; ++r2) st.tau[r2] = (reg == r2 && hi == h) ? nt : st.tau[r2];
        }
    }
}

// The consumer handed to the producers of score_tiles.h: the wavefront's lists of the tile's rows; scores carry no bias.
// init() (the lists' global stores) runs BEHIND the staging of the requested rows: in front of it, the exclusion test's loads of
// o.rows / o.adj_ptr stopped being scalar loads and fp32 with exclude = 1 ran 4 % slower.
// METRIC / CAND: the instance <TK_DOT, false> is gg_topk_scores' consumer -- no scalar load, no bitmap, the scores themselves.
// Under a metric the lane loads ITS column's scalar once per tile (one coalesced 4-byte load per lane) and turns its 16 scores
// into ordering values with one multiply (cosine: s * w_c) or one fmaf (l2: s - h_c / 2) each; everything behind that -- the
// 16 compares with tau, the ballot, the insertion path -- runs on the ordering values unchanged.
template <int METRIC, bool CAND>
struct ListConsumer {
    WaveLists st;
    const TopkOut &o;
    const int r0, sub;
    __device__ __forceinline__ ListConsumer(const TopkOut &o_, int r0_, int sub_) : o(o_), r0(r0_), sub(sub_) {}
    __device__ __forceinline__ void init() { lists_init(st, o, r0, sub); }
    __device__ __forceinline__ float start(int, bool) const { return 0.f; }
    __device__ __forceinline__ void operator()(const f32x16 &acc, int col, bool ok) {
        if (METRIC == TK_DOT) {
            lists_consume<CAND>(st, o, r0, sub, acc, col, ok);
        } else {
            const float cv = ok ? o.colv[col] : 0.f;  // (columns behind the split's end: never a candidate)
            f32x16 t;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) t[reg] = METRIC == TK_COS ? acc[reg] * cv : __builtin_fmaf(-0.5f, cv, acc[reg]);
            lists_consume<CAND>(st, o, r0, sub, t, col, ok);
        }
    }
    __device__ __forceinline__ void operator()(const f32x16 (&acc)[1], int col, bool ok) { (*this)(acc[0], col, ok); }
};

template <int METRIC, bool CAND>
__global__ __launch_bounds__(256) void topk_f32_kernel(const float *E, int n_node, int ld, int cols_per_split, TopkOut o) {
    extern __shared__ float As_all[];  // [32][ld + 1]: the tile's 32 requested rows, staged once
    __shared__ float Bs[128][ST_KC + 1];
    const int split = blockIdx.x, r0 = blockIdx.y * 32, sub = 4 * split + (threadIdx.x >> 6);
    const int cbeg = split * cols_per_split, cend = min(n_node, cbeg + cols_per_split);
    ListConsumer<METRIC, CAND> lists(o, r0, sub);
    f32_score_tiles(E, ld, o.rows, o.n_rows, r0, cbeg, cend, As_all, Bs, lists);
}

// KS k-steps of 16; the next tile's B fragments are prefetched while they fit (KS <= 16).
template <int KS, int METRIC, bool CAND>
__global__ __launch_bounds__(256) void topk_bf16_kernel(const uint4 *Eb, int n_node, int cols_per_split, TopkOut o) {
    const int split = blockIdx.x, r0 = blockIdx.y * 32, sub = 4 * split + (threadIdx.x >> 6);
    const int cbeg = split * cols_per_split, cend = min(n_node, cbeg + cols_per_split);
    ListConsumer<METRIC, CAND> lists(o, r0, sub);
    bf16_score_tiles<KS, 1, (KS <= 16)>(Eb, o.rows, o.n_rows, r0, cbeg, cend, lists);
}

// In place: h_c = |x_c|^2 -> w_c = 1 / sqrt(h_c), a correctly rounded square root and one IEEE division; 0 where h_c == 0
__global__ __launch_bounds__(256) void topk_rsqrt_kernel(float *v, int n) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const float h = v[p];
    v[p] = h == 0.f ? 0.f : 1.0f / __builtin_sqrtf(h);
}

// Count of keys > x in a descending list of k keys.
__device__ __forceinline__ int count_above(const u64 *L, int k, u64 x) {
    int lo = 0, hi = k;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (L[mid] > x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One workgroup per requested row: the row's n_sub lists merged into one k-list in LDS (rank merge: an entry's new position is
// its index plus the entries of the other list above it; keys are distinct), written out as (column, score), -1 / -inf padded.
// Under a metric the keys hold the ordering value t; the reported value is one more fp32 operation with the ROW's scalar
// rowv[rows[row]]: t * w_u (cosine), max(0, h_u - 2 t) (l2: the squared distance, padding +inf).
template <int METRIC>
__global__ __launch_bounds__(256) void topk_merge_kernel(const u64 *part, int n_sub, int k, const int32_t *rows, const float *rowv, int32_t *out_col,
                                                         float *out_score) {
    __shared__ u64 cur[TK_MAX_K], nb[TK_MAX_K];
    __shared__ u64 heads[256];
    const int tid = threadIdx.x, row = blockIdx.x;
    cur[tid] = 0ull;
    const u64 *P = part + (int64_t)row * n_sub * k;
    for (int s0 = 0; s0 < n_sub; s0 += 256) {
        __syncthreads();
        heads[tid] = s0 + tid < n_sub ? P[(int64_t)(s0 + tid) * k] : 0ull;
        __syncthreads();
        const int ns = min(256, n_sub - s0);
        for (int j = 0; j < ns; ++j) {
            if (heads[j] <= cur[k - 1]) continue;  // (uniform: nothing of this list beats the running k-th key; empty lists too)
            const u64 b = tid < k ? P[(int64_t)(s0 + j) * k + tid] : 0ull;
            nb[tid] = b;
            __syncthreads();
            const u64 a = tid < k ? cur[tid] : 0ull;
            const int pa = tid + count_above(nb, k, a), pb = tid + count_above(cur, k, b);
            __syncthreads();
            if (a != 0 && pa < k) cur[pa] = a;
            if (b != 0 && pb < k) cur[pb] = b;
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid < k) {
        const u64 key = cur[tid];
        out_col[(int64_t)row * k + tid] = key ? (int32_t)~(uint32_t)key : -1;
        float x = key ? key_score(key) : -INFINITY;
        if (METRIC == TK_COS) x = key ? x * rowv[rows[row]] : x;
        if (METRIC == TK_L2) x = key ? fmaxf(0.f, __builtin_fmaf(-2.f, x, rowv[rows[row]])) : INFINITY;
        out_score[(int64_t)row * k + tid] = x;
    }
}

}  // namespace

// The resident adjacency with every node's list sorted (binary search of the exclusion test); built on first use after
// gg_set_graph_csr, which drops it.  The resident lists themselves stay in file order (the BFS trees depend on it).  Shared with
// the biased pre-training walks (pretrain.hip: membership in the list of the previous node).
int ensure_sorted_adjacency(gg_ctx *ctx) {
    if (ctx->topk_adj_valid) return GG_OK;
    const int n = ctx->n_node;
    std::vector<int32_t> s(ctx->h_col);
    const int nt = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t)
        th.emplace_back([&, t]() {
            for (int v = (int)((int64_t)n * t / nt); v < (int)((int64_t)n * (t + 1) / nt); ++v)
                std::sort(s.begin() + ctx->h_rowptr[v], s.begin() + ctx->h_rowptr[v + 1]);
        });
    for (auto &x : th) x.join();
    hipError_t e = ctx->topk_adj.reserve(sizeof(int32_t) * std::max<size_t>(s.size(), 1));
    if (e == hipSuccess && !s.empty()) e = hipMemcpy(ctx->topk_adj.p, s.data(), sizeof(int32_t) * s.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "sorted adjacency (%lld entries): %s", (long long)s.size(), hipGetErrorString(e));
    ctx->topk_adj_valid = true;
    return GG_OK;
}

namespace {

// One pass: the tile stream of the precision's instance <METRIC, CAND>, then the merge.
template <int METRIC, bool CAND>
void launch_pass(gg_ctx *ctx, const Model &M, int precision, const Bf16Shape &bs, const uint4 *Eb, size_t dyn, int splits, int cps, const TopkOut &o,
                 int32_t *d_col, float *d_score) {
    const int n = ctx->n_node, ld = ctx->ld;
    const dim3 grid(splits, cdiv(o.n_rows, 32));
    if (precision == 0 && dyn > 48 * 1024) (void)hipFuncSetAttribute((const void *)topk_f32_kernel<METRIC, CAND>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    if (precision == 0) {
        hipLaunchKernelGGL((topk_f32_kernel<METRIC, CAND>), grid, dim3(256), dyn, ctx->stream, M.E, n, ld, cps, o);
    } else if (bs.KS == 4) {
        hipLaunchKernelGGL((topk_bf16_kernel<4, METRIC, CAND>), grid, dim3(256), 0, ctx->stream, Eb, n, cps, o);
    } else if (bs.KS == 8) {
        hipLaunchKernelGGL((topk_bf16_kernel<8, METRIC, CAND>), grid, dim3(256), 0, ctx->stream, Eb, n, cps, o);
    } else if (bs.KS == 16) {
        hipLaunchKernelGGL((topk_bf16_kernel<16, METRIC, CAND>), grid, dim3(256), 0, ctx->stream, Eb, n, cps, o);
    } else {
        hipLaunchKernelGGL((topk_bf16_kernel<32, METRIC, CAND>), grid, dim3(256), 0, ctx->stream, Eb, n, cps, o);
    }
    hipLaunchKernelGGL(topk_merge_kernel<METRIC>, dim3(o.n_rows), dim3(256), 0, ctx->stream, (const u64 *)o.part, o.n_sub, o.k, o.rows, o.colv, d_col, d_score);
}

// gg_topk_scores (fn names it; metric = dot, no candidate set, exclude 0 / 1: the instance <TK_DOT, false>) and gg_topk_metric.
int topk_run(gg_ctx *ctx, const char *fn, int32_t which, const int32_t *rows, int32_t n_rows, int32_t k, int32_t precision, int32_t metric,
             int32_t exclude, int32_t max_exclude, const int32_t *cand_nodes, int64_t n_cand, int32_t *out_col, float *out_score, double *kernel_ms_out) {
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    GG_CHECK(ctx, which == 0 || which == 1, GG_EINVAL, "%s: which must be 0 (generator) or 1 (discriminator)", fn);
    GG_CHECK(ctx, k >= 1 && k <= TK_MAX_K, GG_EINVAL, "%s: k = %d outside [1, %d]", fn, k, TK_MAX_K);
    GG_CHECK(ctx, precision == 0 || precision == 1, GG_EINVAL, "%s: precision must be 0 (fp32) or 1 (bf16)", fn);
    GG_CHECK(ctx, metric == TK_DOT || metric == TK_COS || metric == TK_L2, GG_EINVAL, "%s: metric must be 0 (dot), 1 (cosine) or 2 (l2)", fn);
    if (max_exclude == 1) GG_CHECK(ctx, exclude == 0 || exclude == 1, GG_EINVAL, "%s: exclude must be 0 or 1", fn);
    else GG_CHECK(ctx, exclude >= 0 && exclude <= 2, GG_EINVAL, "%s: exclude must be 0, 1 (self and training neighbours) or 2 (self)", fn);
    GG_CHECK(ctx, out_col && out_score && (rows || n_rows >= 0) && n_rows >= 0, GG_EINVAL, "%s: bad argument", fn);
    GG_CHECK(ctx, !cand_nodes || n_cand >= 0, GG_EINVAL, "%s: n_cand = %lld is negative", fn, (long long)n_cand);
    GG_CHECK(ctx, exclude != 1 || ctx->g_rowptr, GG_EINVAL, "%s: exclude = 1 needs the training graph (gg_set_graph_csr)", fn);
    const int n = ctx->n_node, ld = ctx->ld;
    GG_CHECK(ctx, precision == 0 || ctx->n_emb <= 512, GG_EINVAL, "%s: bf16 supports n_emb <= 512 (got %d)", fn, ctx->n_emb);
    const size_t dyn = sizeof(float) * 32 * (size_t)(ld + 1);
    GG_CHECK(ctx, precision == 1 || dyn <= 140 * 1024, GG_EINVAL, "%s: fp32 supports n_emb <= 1116 (got %d)", fn, ctx->n_emb);
    if (!rows) n_rows = n;
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    if (max_exclude == 1) {
        if (const int rc = check_row_ids(ctx, fn, rows, n_rows)) return rc;
    } else {
        if (rows)
            for (int i = 0; i < n_rows; ++i)
                GG_CHECK(ctx, rows[i] >= 0 && rows[i] < n, GG_EINVAL, "%s: rows[%d] = %d out of range [0, %d)", fn, i, rows[i], n);
        if (cand_nodes)
            for (int64_t i = 0; i < n_cand; ++i)
                GG_CHECK(ctx, cand_nodes[i] >= 0 && cand_nodes[i] < n, GG_EINVAL, "%s: cand_nodes[%lld] = %d out of range [0, %d)", fn, (long long)i,
                         cand_nodes[i], n);
    }
    if (n_rows == 0) return GG_OK;
    GG_HIP(ctx, hipSetDevice(ctx->device));
    if (exclude == 1) {
        const int rc = ensure_sorted_adjacency(ctx);
        if (rc != GG_OK) return rc;
    }
    // the instances with a bitmap also carry exclude = 2's test; without a candidate set they get the full set
    const bool bitmap = cand_nodes != nullptr || exclude == 2;
    const int n_words = cdiv(n, 32);
    std::vector<uint32_t> member;
    if (bitmap) {
        member.assign(n_words, cand_nodes ? 0u : 0xffffffffu);
        if (cand_nodes)
            for (int64_t i = 0; i < n_cand; ++i) member[cand_nodes[i] >> 5] |= 1u << (cand_nodes[i] & 31);
    }
    const Bf16Shape bs = bf16_shape(ctx->n_emb);
    const int chunk = std::min(n_rows, TK_CHUNK);
    // column splits as K7's, the partial lists of a pass (4 per split and row) within TK_PART_CAP
    const ColumnSplit cs = column_split(n, cdiv(chunk, 32), 2048, (int)(TK_PART_CAP / ((size_t)chunk * 4 * k * sizeof(u64))));
    const int splits = cs.splits, cps = cs.cols_per_split, n_sub = 4 * splits;
    const Model &M = ctx->model[which];
    DevBuf d_rows, d_part, d_col, d_score, d_bf, d_colv, d_member;
    auto rel = [&]() { d_rows.release(); d_part.release(); d_col.release(); d_score.release(); d_bf.release(); d_colv.release(); d_member.release(); };
    hipError_t e = d_rows.reserve(sizeof(int32_t) * chunk);
    if (e == hipSuccess) e = d_part.reserve(sizeof(u64) * (size_t)chunk * n_sub * k);
    if (e == hipSuccess) e = d_col.reserve(sizeof(int32_t) * (size_t)chunk * k);
    if (e == hipSuccess) e = d_score.reserve(sizeof(float) * (size_t)chunk * k);
    if (e == hipSuccess && precision == 1) e = bf16_table(ctx, which, bs.ld16, d_bf);
    if (e == hipSuccess && metric != TK_DOT) e = d_colv.reserve(sizeof(float) * (size_t)n);
    if (e == hipSuccess && bitmap) e = d_member.reserve(sizeof(uint32_t) * (size_t)n_words);
    if (e != hipSuccess) { rel(); return fail(ctx, GG_ENOMEM, "%s: %s", fn, hipGetErrorString(e)); }
    if (bitmap) e = hipMemcpyAsync(d_member.p, member.data(), sizeof(uint32_t) * (size_t)n_words, hipMemcpyHostToDevice, ctx->stream);
    std::vector<int32_t> ids;
    double ms_total = 0.0;
    for (int c0 = 0; c0 < n_rows && e == hipSuccess; c0 += chunk) {
        const int cr = std::min(chunk, n_rows - c0);
        const int32_t *src = rows ? rows + c0 : nullptr;
        if (!rows) {
            ids.resize(cr);
            for (int i = 0; i < cr; ++i) ids[i] = c0 + i;
            src = ids.data();
        }
        e = hipMemcpyAsync(d_rows.p, src, sizeof(int32_t) * cr, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) break;
        TopkOut o{d_rows.as<int32_t>(), cr, k, exclude == 1 ? ctx->g_rowptr : nullptr, exclude == 1 ? ctx->topk_adj.as<int32_t>() : nullptr, d_part.as<u64>(), n_sub,
                  d_colv.as<float>(), d_member.as<uint32_t>(), exclude == 2 ? 1 : 0};
        (void)hipEventRecord(ctx->ev0, ctx->stream);
        if (c0 == 0 && metric != TK_DOT) {  // h (and from it w) of all columns, once per call, in front of the passes
            if (precision == 0) hipLaunchKernelGGL(sil_norm_kernel<false>, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, M.E, ld, (const int32_t *)nullptr, n, d_colv.as<float>());
            else hipLaunchKernelGGL(sil_norm_kernel<true>, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, M.E, ld, (const int32_t *)nullptr, n, d_colv.as<float>());
            if (metric == TK_COS) hipLaunchKernelGGL(topk_rsqrt_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, d_colv.as<float>(), n);
        }
        const uint4 *Eb = (const uint4 *)d_bf.p;
        int32_t *oc = d_col.as<int32_t>();
        float *os = d_score.as<float>();
        if (metric == TK_DOT && !bitmap) launch_pass<TK_DOT, false>(ctx, M, precision, bs, Eb, dyn, splits, cps, o, oc, os);
        else if (metric == TK_DOT) launch_pass<TK_DOT, true>(ctx, M, precision, bs, Eb, dyn, splits, cps, o, oc, os);
        else if (metric == TK_COS && !bitmap) launch_pass<TK_COS, false>(ctx, M, precision, bs, Eb, dyn, splits, cps, o, oc, os);
        else if (metric == TK_COS) launch_pass<TK_COS, true>(ctx, M, precision, bs, Eb, dyn, splits, cps, o, oc, os);
        else if (!bitmap) launch_pass<TK_L2, false>(ctx, M, precision, bs, Eb, dyn, splits, cps, o, oc, os);
        else launch_pass<TK_L2, true>(ctx, M, precision, bs, Eb, dyn, splits, cps, o, oc, os);
        (void)hipEventRecord(ctx->ev1, ctx->stream);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(out_col + (int64_t)c0 * k, d_col.p, sizeof(int32_t) * (size_t)cr * k, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(out_score + (int64_t)c0 * k, d_score.p, sizeof(float) * (size_t)cr * k, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        float ms = 0.f;
        if (e == hipSuccess) (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
        ms_total += ms;
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(ctx->stream);  // (the bitmap's source and the buffers go away behind it)
    rel();
    if (e != hipSuccess) return fail(ctx, GG_EHIP, "%s: %s", fn, hipGetErrorString(e));
    if (kernel_ms_out) *kernel_ms_out = ms_total;
    return GG_OK;
}

}  // namespace

}  // namespace gg

using namespace gg;

// gg_topk_scores: see include/graphgan_hip.h.
extern "C" int gg_topk_scores(gg_ctx *ctx, int32_t which, const int32_t *rows, int32_t n_rows, int32_t k, int32_t precision, int32_t exclude,
                              int32_t *out_col, float *out_score, double *kernel_ms_out) {
    return topk_run(ctx, "gg_topk_scores", which, rows, n_rows, k, precision, TK_DOT, exclude, 1, nullptr, 0, out_col, out_score, kernel_ms_out);
}

// gg_topk_metric: see include/graphgan_hip.h.
extern "C" int gg_topk_metric(gg_ctx *ctx, int32_t which, const int32_t *rows, int32_t n_rows, int32_t k, int32_t precision, int32_t metric, int32_t exclude,
                              const int32_t *cand_nodes, int64_t n_cand, int32_t *out_col, float *out_score, double *kernel_ms_out) {
    return topk_run(ctx, "gg_topk_metric", which, rows, n_rows, k, precision, metric, exclude, 2, cand_nodes, n_cand, out_col, out_score, kernel_ms_out);
}

