// two_hop.hip -- the two-hop sweep behind the graph-only ranking baselines: per query u one row of A W A on the resident training
// graph, S(u, c) = sum over w in N(u) & N(c) of weights[w] (unsigned 64-bit integers; no weights: common neighbours), and from
// it either the best k candidates (gg_two_hop_topk) or the integers that place one target in the total order (gg_two_hop_rank).
// No embedding table is read: integer gathers over the SET adjacency of ensure_set_adjacency (pair_neighbors.hip).  The kernels
// hold no floating-point operation.
//
// Shape (the first build; what was not tuned is listed in DESIGN.md "Two-hop sweep").  The host plans per query from the host
// copy of the set adjacency: T(u) = sum over w in N(u) of deg(w), the entries of the expansion.  One workgroup per query:
//   fill        a (column, uint64 sum) SetTable (set_sweep.h) for min(T, n_node) entries.  T <= TH_LDS_CAP = 2048: the table lies
//               in LDS (4096 slots x 12 B = 48 KiB, with the selection's buffers 52 KiB: three workgroups share a CU's
//               160 KiB); above, in a zeroed table of the context's scratch buffer (per task the values, then the keys), the
//               queries batched under scratch_bytes.
//               Lists N(w) of up to TH_NARROW = 64 entries are walked by groups of 16 lanes (16 lists at a time), longer ones
//               by all 256 lanes of the workgroup: no list is truncated and no lane walks a hub's list alone;
//   rank        set_rank_consume (set_consume.h, shared with the push sweep): the target's slot is looked up and the table is
//               scanned once, counting n_pos, ahead and pos_below with compares;
//   top-K       set_topk_consume: the ineligible entries are zeroed in place, a radix select on the composite key (score,
//               ~column) finds the k-th largest, and the min(k, n_pos) survivors are bitonic-sorted in LDS.
// Every sum is an integer and the order is total, so a query's outputs depend on the graph, the weights and the query alone --
// not on the request, the grid, the batches, the order of the inserts or the run.
#include <algorithm>

#include "set_consume.h"

namespace gg {

namespace {

constexpr int TH_LDS_CAP = 2048;      // expansion entries T the LDS table takes (Engine.TWO_HOP_LDS_CAP); larger queries use global memory
constexpr int TH_LDS_SLOTS = 2 * TH_LDS_CAP;
constexpr int TH_MAX_K = 256;         // list length at most: the survivors are sorted by one workgroup of 256 threads
static_assert(TH_MAX_K == SET_MAX_K, "the shared top-K consumer sorts TH_MAX_K survivors");
constexpr int TH_NARROW = 64;         // a list N(w) up to this length is walked by a 16-lane group, a longer one by the workgroup
constexpr int TH_BLOCKS = 2048;       // workgroups per launch at most; they stride over the tasks behind them
constexpr int64_t TH_SCRATCH = 256ll << 20;  // default cap on the global tables of one pass, bytes
constexpr int64_t TH_CHUNK_OUT = 1ll << 23;  // list entries (queries x k) of one chunk of a top-K request at most

struct ThTask {
    int32_t q;        // query of the chunk
    uint32_t slots;   // table size, a power of two
    int64_t off;      // global table: first 8-byte word of the task's table in tab (slots values, then slots key words)
};

struct ThArgs {
    const ThTask *task;
    int n_task;
    unsigned long long *tab;          // zeroed global tables of the pass
    const int32_t *u, *v;             // [chunk] query nodes; targets (rank only)
    const int64_t *ptr;               // set adjacency
    const int32_t *adj;
    const unsigned long long *w;      // [n_node] or NULL: every weight 1
    int excl;                         // 1: c != u; 2: c outside N(u) + {u}
    int k;
    int32_t *out_col;                 // top-K: [chunk, k]
    unsigned long long *out_score;    //        [chunk, k]
    int32_t *n_pos;                   // [chunk]
    unsigned long long *score;        // rank: [chunk]
    int32_t *ahead, *pos_below;       //       [chunk]
};

template <bool GLOBAL>
using ThTab = SetTable<unsigned long long, GLOBAL>;  // at most min(T, n_node) distinct columns in >= twice as many slots

// the expansion of u into the table; every thread of the workgroup calls it (barrier inside)
template <bool GLOBAL>
__device__ __forceinline__ void th_fill(const ThArgs &o, const ThTab<GLOBAL> &tb, int64_t ub, int du) {
    const int tid = threadIdx.x, gl = tid & 15;
    int wide = 0;
    for (int j = tid >> 4; j < du; j += 16) {
        const int w = o.adj[ub + j];
        const int64_t wb = o.ptr[w];
        const int dw = (int)(o.ptr[w + 1] - wb);
        if (dw > TH_NARROW) {
            wide = 1;
            continue;
        }
        const unsigned long long wv = o.w ? o.w[w] : 1ull;
        for (int e = gl; e < dw; e += 16) tb.add(o.adj[wb + e], wv);
    }
    if (__syncthreads_or(wide)) {  // (block-uniform)
        for (int j = 0; j < du; ++j) {
            const int w = o.adj[ub + j];
            const int64_t wb = o.ptr[w];
            const int dw = (int)(o.ptr[w + 1] - wb);
            if (dw <= TH_NARROW) continue;
            const unsigned long long wv = o.w ? o.w[w] : 1ull;
            for (int e = tid; e < dw; e += 256) tb.add(o.adj[wb + e], wv);
        }
    }
    tb.fill_done();
}

template <bool GLOBAL>
__global__ __launch_bounds__(256) void th_rank_kernel(ThArgs o) {
    __shared__ uint32_t s_key[GLOBAL ? 1 : TH_LDS_SLOTS];
    __shared__ unsigned long long s_val[GLOBAL ? 1 : TH_LDS_SLOTS];
    const int tid = threadIdx.x;
    for (int t = blockIdx.x; t < o.n_task; t += gridDim.x) {  // (block-uniform: the barriers below are reached by every thread)
        const ThTask tk = o.task[t];
        const int i = tk.q, u = o.u[i], v = o.v[i];
        ThTab<GLOBAL> tb;
        tb.val = GLOBAL ? o.tab + tk.off : s_val;
        tb.key = GLOBAL ? (uint32_t *)(tb.val + tk.slots) : s_key;
        tb.mask = tk.slots - 1u;
        if (!GLOBAL) tb.clear_lds();
        const int64_t ub = o.ptr[u];
        const int du = (int)(o.ptr[u + 1] - ub);
        th_fill<GLOBAL>(o, tb, ub, du);
        unsigned long long sv;
        int np, ah, below;
        set_rank_consume<GLOBAL>(tb, tk.slots, u, v, o.adj + ub, du, o.excl, sv, np, ah, below);
        if (tid == 0) {
            o.score[i] = sv;
            o.n_pos[i] = np;
            o.ahead[i] = ah;
            o.pos_below[i] = below;
        }
        __syncthreads();  // (the next task clears the table and the fold words)
    }
}

template <bool GLOBAL>
__global__ __launch_bounds__(256) void th_topk_kernel(ThArgs o) {
    __shared__ uint32_t s_key[GLOBAL ? 1 : TH_LDS_SLOTS];
    __shared__ unsigned long long s_val[GLOBAL ? 1 : TH_LDS_SLOTS];
    const int tid = threadIdx.x;
    for (int t = blockIdx.x; t < o.n_task; t += gridDim.x) {  // (block-uniform: the barriers below are reached by every thread)
        const ThTask tk = o.task[t];
        const int i = tk.q, u = o.u[i];
        ThTab<GLOBAL> tb;
        tb.val = GLOBAL ? o.tab + tk.off : s_val;
        tb.key = GLOBAL ? (uint32_t *)(tb.val + tk.slots) : s_key;
        tb.mask = tk.slots - 1u;
        if (!GLOBAL) tb.clear_lds();
        const int64_t ub = o.ptr[u];
        const int du = (int)(o.ptr[u + 1] - ub);
        th_fill<GLOBAL>(o, tb, ub, du);
        set_topk_consume<GLOBAL>(tb, tk.slots, u, o.adj + ub, du, o.excl, o.k, (int64_t)i, o.out_col, o.out_score, o.n_pos);
        __syncthreads();  // (the next task clears the table, the list and the fold words)
    }
}

// The sweep of one request: `rank` selects the outputs.  Queries go in chunks (bounded device memory for the outputs); within a
// chunk the LDS-table queries are one launch and the global-table queries as many passes as scratch_bytes asks for (a pass takes
// at least one query, whatever its table's size).
int th_run(gg_ctx *ctx, const char *fn, bool rank, const int32_t *u, const int32_t *v, int64_t m, int k, const uint64_t *weights, int excl, int64_t scratch_bytes,
           int32_t *out_col, uint64_t *out_score, uint64_t *score, int32_t *ahead, int32_t *n_pos, int32_t *pos_below, double *kernel_ms) {
    const int n = ctx->n_node;
    GG_HIP(ctx, hipSetDevice(ctx->device));
    int rc = ensure_set_adjacency(ctx);
    if (rc == GG_OK && weights) rc = check_weight_bound(ctx, fn, weights, n);
    if (rc != GG_OK) return rc;
    const int64_t cap = scratch_bytes > 0 ? scratch_bytes : TH_SCRATCH;
    const int64_t *hp = ctx->set.h_ptr.data();
    const int32_t *ha = ctx->set.h_adj.data();
    const int64_t chunk = rank ? std::min<int64_t>(m, 1 << 20) : std::min<int64_t>(m, std::max<int64_t>(1, TH_CHUNK_OUT / k));
    ScopedBuf d_u, d_v, d_w, d_task, d_col, d_sc, d_np, d_ah, d_below;
    hipError_t e = d_u.reserve(sizeof(int32_t) * (size_t)chunk);
    if (e == hipSuccess) e = d_np.reserve(sizeof(int32_t) * (size_t)chunk);
    if (e == hipSuccess) e = d_task.reserve(sizeof(ThTask) * (size_t)chunk);
    if (rank) {
        for (ScopedBuf *b : {&d_v, &d_ah, &d_below})
            if (e == hipSuccess) e = b->reserve(sizeof(int32_t) * (size_t)chunk);
        if (e == hipSuccess) e = d_sc.reserve(sizeof(uint64_t) * (size_t)chunk);
    } else {
        if (e == hipSuccess) e = d_col.reserve(sizeof(int32_t) * (size_t)chunk * k);
        if (e == hipSuccess) e = d_sc.reserve(sizeof(uint64_t) * (size_t)chunk * k);
    }
    if (e == hipSuccess && weights) e = d_w.reserve(sizeof(uint64_t) * (size_t)n);
    if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "%s: %s", fn, hipGetErrorString(e));
    if (weights) GG_HIP_FN(hipMemcpyAsync(d_w.p, weights, sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    std::vector<ThTask> task;
    std::vector<int64_t> expansion;   // T(u) of the chunk's queries
    std::vector<int64_t> pass_first;  // global-table passes: first task of each, then the end
    double ms_total = 0.0;
    for (int64_t p0 = 0; p0 < m; p0 += chunk) {
        const int cr = (int)std::min<int64_t>(chunk, m - p0);
        // the chunk's tasks: the LDS-table queries first, then the global-table queries cut into passes
        task.assign((size_t)cr, ThTask{});
        expansion.resize((size_t)cr);
        for (int i = 0; i < cr; ++i) {
            const int a = u[p0 + i];
            int64_t T = 0;
            for (int64_t j = hp[a]; j < hp[a + 1]; ++j) T += hp[ha[j] + 1] - hp[ha[j]];
            expansion[(size_t)i] = T;
        }
        int n_lds = 0, n_glob = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (int i = 0; i < cr; ++i) {
                const int64_t T = expansion[(size_t)i];
                const bool lds = T <= TH_LDS_CAP;
                if (lds != (pass == 0)) continue;
                ThTask &tk = task[(size_t)(lds ? n_lds++ : n_lds + n_glob++)];
                tk.q = i;
                tk.slots = (uint32_t)set_table_slots(std::min<int64_t>(T, n));
            }
        pass_first.assign(1, n_lds);
        int64_t words = 0, max_words = 0;
        for (int t = n_lds; t < cr; ++t) {
            const int64_t need = (int64_t)task[t].slots + task[t].slots / 2;  // 8-byte words: the values, then the 4-byte keys
            if (words && (words + need) * 8 > cap) {
                pass_first.push_back(t);
                words = 0;
            }
            task[t].off = words;
            words += need;
            max_words = std::max(max_words, words);
        }
        pass_first.push_back(cr);
        if (max_words) {
            e = ctx->set.th_tab.reserve(sizeof(uint64_t) * (size_t)max_words);
            if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "%s: %lld bytes of table scratch: %s", fn, (long long)(max_words * 8), hipGetErrorString(e));
        }
        GG_HIP_FN(hipMemcpyAsync(d_u.p, u + p0, sizeof(int32_t) * cr, hipMemcpyHostToDevice, ctx->stream));
        if (rank) GG_HIP_FN(hipMemcpyAsync(d_v.p, v + p0, sizeof(int32_t) * cr, hipMemcpyHostToDevice, ctx->stream));
        GG_HIP_FN(hipMemcpyAsync(d_task.p, task.data(), sizeof(ThTask) * (size_t)cr, hipMemcpyHostToDevice, ctx->stream));
        ThArgs o{};
        o.tab = ctx->set.th_tab.as<unsigned long long>();
        o.u = d_u.as<int32_t>();
        o.v = d_v.as<int32_t>();
        o.ptr = ctx->set.ptr.as<int64_t>();
        o.adj = ctx->set.adj.as<int32_t>();
        o.w = weights ? d_w.as<unsigned long long>() : nullptr;
        o.excl = excl;
        o.k = k;
        o.out_col = d_col.as<int32_t>();
        o.out_score = rank ? nullptr : d_sc.as<unsigned long long>();
        o.score = rank ? d_sc.as<unsigned long long>() : nullptr;
        o.n_pos = d_np.as<int32_t>();
        o.ahead = d_ah.as<int32_t>();
        o.pos_below = d_below.as<int32_t>();
        (void)hipEventRecord(ctx->ev0, ctx->stream);
        if (n_lds) {
            o.task = d_task.as<ThTask>();
            o.n_task = n_lds;
            const dim3 grid((unsigned)std::min(TH_BLOCKS, n_lds));
            if (rank) hipLaunchKernelGGL(th_rank_kernel<false>, grid, dim3(256), 0, ctx->stream, o);
            else hipLaunchKernelGGL(th_topk_kernel<false>, grid, dim3(256), 0, ctx->stream, o);
        }
        for (size_t ps = 0; ps + 1 < pass_first.size(); ++ps) {
            const int64_t t0 = pass_first[ps], t1 = pass_first[ps + 1];
            if (t1 == t0) continue;
            const int64_t used = task[(size_t)t1 - 1].off + task[(size_t)t1 - 1].slots + task[(size_t)t1 - 1].slots / 2;
            GG_HIP_FN(hipMemsetAsync(ctx->set.th_tab.p, 0, sizeof(uint64_t) * (size_t)used, ctx->stream));
            o.task = d_task.as<ThTask>() + t0;
            o.n_task = (int)(t1 - t0);
            const dim3 grid((unsigned)std::min<int64_t>(TH_BLOCKS, t1 - t0));
            if (rank) hipLaunchKernelGGL(th_rank_kernel<true>, grid, dim3(256), 0, ctx->stream, o);
            else hipLaunchKernelGGL(th_topk_kernel<true>, grid, dim3(256), 0, ctx->stream, o);
        }
        (void)hipEventRecord(ctx->ev1, ctx->stream);
        GG_HIP_FN(hipGetLastError());
        GG_HIP_FN(hipMemcpyAsync(n_pos + p0, d_np.p, sizeof(int32_t) * cr, hipMemcpyDeviceToHost, ctx->stream));
        if (rank) {
            GG_HIP_FN(hipMemcpyAsync(score + p0, d_sc.p, sizeof(uint64_t) * cr, hipMemcpyDeviceToHost, ctx->stream));
            GG_HIP_FN(hipMemcpyAsync(ahead + p0, d_ah.p, sizeof(int32_t) * cr, hipMemcpyDeviceToHost, ctx->stream));
            GG_HIP_FN(hipMemcpyAsync(pos_below + p0, d_below.p, sizeof(int32_t) * cr, hipMemcpyDeviceToHost, ctx->stream));
        } else {
            GG_HIP_FN(hipMemcpyAsync(out_col + p0 * k, d_col.p, sizeof(int32_t) * (size_t)cr * k, hipMemcpyDeviceToHost, ctx->stream));
            GG_HIP_FN(hipMemcpyAsync(out_score + p0 * k, d_sc.p, sizeof(uint64_t) * (size_t)cr * k, hipMemcpyDeviceToHost, ctx->stream));
        }
        GG_HIP_FN(hipStreamSynchronize(ctx->stream));
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
        ms_total += ms;
    }
    if (kernel_ms) *kernel_ms = ms_total;
    return GG_OK;
}

}  // namespace

}  // namespace gg

using namespace gg;

// gg_two_hop_topk, gg_two_hop_rank: see include/graphgan_hip.h.
extern "C" int gg_two_hop_topk(gg_ctx *ctx, const int32_t *rows, int64_t n_rows, int32_t k, const uint64_t *weights, int32_t exclude, int64_t scratch_bytes,
                               int32_t *out_col, uint64_t *out_score, int32_t *n_pos, double *kernel_ms) {
    const char *fn = "gg_two_hop_topk";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (kernel_ms) *kernel_ms = 0.0;
    const int rc = check_query_request(ctx, fn, n_rows, "n_rows", exclude, scratch_bytes);
    if (rc != GG_OK) return rc;
    GG_CHECK(ctx, k >= 1 && k <= TH_MAX_K, GG_EINVAL, "%s: k = %d outside [1, %d]", fn, k, TH_MAX_K);
    if (n_rows == 0) return GG_OK;
    GG_CHECK(ctx, rows && out_col && out_score && n_pos, GG_EINVAL, "%s: rows, out_col, out_score and n_pos must not be NULL", fn);
    const int rc2 = check_ids(ctx, fn, "rows", rows, n_rows);
    if (rc2 != GG_OK) return rc2;
    return th_run(ctx, fn, false, rows, nullptr, n_rows, k, weights, exclude, scratch_bytes, out_col, out_score, nullptr, nullptr, n_pos, nullptr, kernel_ms);
}

extern "C" int gg_two_hop_rank(gg_ctx *ctx, const int32_t *u, const int32_t *v, int64_t m, const uint64_t *weights, int32_t exclude, int64_t scratch_bytes,
                               uint64_t *score, int32_t *ahead, int32_t *n_pos, int32_t *pos_below, double *kernel_ms) {
    const char *fn = "gg_two_hop_rank";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (kernel_ms) *kernel_ms = 0.0;
    const int rc = check_query_request(ctx, fn, m, "m", exclude, scratch_bytes);
    if (rc != GG_OK) return rc;
    if (m == 0) return GG_OK;
    GG_CHECK(ctx, u && v && score && ahead && n_pos && pos_below, GG_EINVAL, "%s: u, v, score, ahead, n_pos and pos_below must not be NULL", fn);
    int rc2 = check_ids(ctx, fn, "u", u, m);
    if (rc2 == GG_OK) rc2 = check_ids(ctx, fn, "v", v, m);
    if (rc2 != GG_OK) return rc2;
    return th_run(ctx, fn, true, u, v, m, 1, weights, exclude, scratch_bytes, nullptr, nullptr, score, ahead, n_pos, pos_below, kernel_ms);
}
