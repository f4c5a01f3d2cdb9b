// pair_neighbors.hip -- the pair-neighbour sweep behind the neighbourhood link-prediction indices (common neighbours, Jaccard,
// Adamic-Adar, resource allocation, preferential attachment): for each pair (u, v) the size of C(u, v) = (N(u) & N(v)) \ {u, v}
// in the resident training graph, the two distinct degrees, and up to four sums of per-node unsigned 64-bit weights over C(u, v).
// No embedding table is read: a latency-bound integer gather, not a tile stream.
//
// The sweep runs on the SET adjacency (ensure_set_adjacency): every node's list sorted, distinct and without the node itself,
// under row offsets of its own, so deg(x) is an offset difference and membership is a binary search.
//
// Work is a list of TASKS the host plans from the degrees, one kernel launch per group width W in {4, 16, 64}:
//   a task      (pair, first entry c0) = the entries [c0, min(len, c0 + PN_CHUNK)) of the pair's SHORTER list;
//   a group     W adjacent lanes take a task: lane l walks the entries c0 + l, c0 + l + W, ... and looks each one up in the
//               longer list.  A lane's entries ascend, so each search starts where the lane's previous one ended;
//   W           from the shorter list's length s: s <= 8 -> 4, s <= 64 -> 16, else 64 (a whole wavefront per pair would idle
//               on a graph of mean degree 5) -- the planner and the launcher of set_sweep.h;
//   a long pair s > PN_CHUNK: ceil(s / PN_CHUNK) tasks at W = 64 -- one wavefront never walks a hub's whole list -- which ADD
//               their partial results into the zeroed outputs with integer atomics.  Every other pair has one task, which
//               stores.
// Integer partials are folded over the group by shuffles.  All sums are integers, so neither the split, the order of the adds
// nor which list is walked changes a bit of the result.
#include <algorithm>
#include <thread>

#include "set_sweep.h"

namespace gg {

namespace {

constexpr int PN_CHUNK = 512;          // entries of the shorter list per task (Engine.PAIR_NEIGHBORS_CHUNK)
constexpr int PN_MAX_W = 4;            // weight arrays per call at most
constexpr int PN_BLOCKS = 2048;        // workgroups per launch at most (8 per CU); the groups stride over the tasks behind them
constexpr int64_t PN_PASS = 1 << 22;   // pairs per internal pass (bounds the temporary device memory)

struct PnArgs {
    const int32_t *u, *v;       // [n] the pass's pairs
    int n;                      // pairs of the pass: the stride of wsum
    const int2 *task;           // [n_task] (pair, c0) of this launch
    int n_task;
    const int64_t *ptr;         // set adjacency
    const int32_t *adj;
    const uint64_t *w;          // [n_w * n_node]
    int n_w, n_node;
    int32_t *cn, *deg_u, *deg_v;   // [n]
    unsigned long long *wsum;      // [n_w * n]
};

template <int W>
__global__ __launch_bounds__(256) void pn_sweep_kernel(PnArgs o) {
    const int gl = threadIdx.x & (W - 1);
    const int groups = gridDim.x * (256 / W);
    for (int t = blockIdx.x * (256 / W) + threadIdx.x / W; t < o.n_task; t += groups) {  // (the same trip count in every lane of a group)
        const int2 tk = o.task[t];
        const int i = tk.x, c0 = tk.y;
        const int u = o.u[i], v = o.v[i];
        const int64_t ub = o.ptr[u], vb = o.ptr[v];
        const int ulen = (int)(o.ptr[u + 1] - ub), vlen = (int)(o.ptr[v + 1] - vb);
        const bool u_short = ulen <= vlen;
        const int32_t *A = o.adj + (u_short ? ub : vb), *B = o.adj + (u_short ? vb : ub);  // walked, searched
        const int alen = u_short ? ulen : vlen, blen = u_short ? vlen : ulen;
        const int end = min(alen, c0 + PN_CHUNK);
        int cnt = 0, lo = 0;
        unsigned long long ws[PN_MAX_W] = {0ull, 0ull, 0ull, 0ull};
        for (int e = c0 + gl; e < end; e += W) {
            const int x = A[e];
            lo = set_lower_bound(B, lo, blen, x);  // from the lane's previous position on
            if (lo < blen && B[lo] == x && x != u && x != v) {
                ++cnt;
#pragma unroll
                for (int j = 0; j < PN_MAX_W; ++j)
                    if (j < o.n_w) ws[j] += o.w[(int64_t)j * o.n_node + x];
            }
        }
#pragma unroll
        for (int off = W / 2; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, W);
#pragma unroll
        for (int j = 0; j < PN_MAX_W; ++j)
            if (j < o.n_w) {
#pragma unroll
                for (int off = W / 2; off >= 1; off >>= 1) ws[j] += __shfl_xor(ws[j], off, W);
            }
        if (gl == 0) {
            if (c0 == 0) {
                o.deg_u[i] = ulen;
                o.deg_v[i] = vlen;
            }
            if (alen <= PN_CHUNK) {  // the pair's only task
                o.cn[i] = cnt;
#pragma unroll
                for (int j = 0; j < PN_MAX_W; ++j)
                    if (j < o.n_w) o.wsum[(int64_t)j * o.n + i] = ws[j];
            } else {  // one of several: the outputs were zeroed
                if (cnt) atomicAdd(o.cn + i, cnt);
#pragma unroll
                for (int j = 0; j < PN_MAX_W; ++j)
                    if (j < o.n_w && ws[j]) atomicAdd(o.wsum + (int64_t)j * o.n + i, ws[j]);
            }
        }
    }
}

}  // namespace

// The set adjacency of the resident graph: per node the sorted distinct neighbours other than the node itself, under int64 row
// offsets of its own (ctx->set, with host copies).  Built on first use after gg_set_graph_csr, which drops it; the resident lists and
// the sorted copy of ensure_sorted_adjacency (which keeps duplicates and self-loops) are not touched.
int ensure_set_adjacency(gg_ctx *ctx) {
    SetGraph &g = ctx->set;
    if (g.valid) return GG_OK;
    const int n = ctx->n_node;
    std::vector<int32_t> s(ctx->h_col);
    std::vector<int64_t> &ptr = g.h_ptr;
    ptr.assign((size_t)n + 1, 0);
    const int nt = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t)
        th.emplace_back([&, t]() {
            for (int v = (int)((int64_t)n * t / nt); v < (int)((int64_t)n * (t + 1) / nt); ++v) {
                auto b = s.begin() + ctx->h_rowptr[v], e = s.begin() + ctx->h_rowptr[v + 1];
                std::sort(b, e);
                e = std::remove(b, std::unique(b, e), v);
                ptr[v + 1] = e - b;
            }
        });
    for (auto &x : th) x.join();
    int64_t max_deg = 0;
    for (int v = 0; v < n; ++v) {  // counts -> offsets, and the lists moved together (a list only ever moves towards the front)
        const int64_t len = ptr[v + 1];
        max_deg = std::max(max_deg, len);
        std::copy(s.begin() + ctx->h_rowptr[v], s.begin() + ctx->h_rowptr[v] + len, s.begin() + ptr[v]);
        ptr[v + 1] = ptr[v] + len;
    }
    const size_t total = (size_t)ptr[n];
    hipError_t e = g.ptr.reserve(sizeof(int64_t) * ((size_t)n + 1));
    if (e == hipSuccess) e = g.adj.reserve(sizeof(int32_t) * std::max<size_t>(total, 1));
    if (e == hipSuccess) e = hipMemcpy(g.ptr.p, ptr.data(), sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess && total) e = hipMemcpy(g.adj.p, s.data(), sizeof(int32_t) * total, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "set adjacency (%lld entries): %s", (long long)total, hipGetErrorString(e));
    s.resize(total);
    g.h_adj.swap(s);  // (the host copy of the lists: the two-hop sweep plans its queries from it, two_hop.hip)
    g.max_deg = (int32_t)max_deg;
    g.valid = true;
    return GG_OK;
}

}  // namespace gg

using namespace gg;

// gg_distinct_degrees, gg_pair_neighbors: see include/graphgan_hip.h.
extern "C" int gg_distinct_degrees(gg_ctx *ctx, int32_t *deg) {
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    GG_CHECK(ctx, ctx->g_rowptr, GG_EINVAL, "gg_distinct_degrees: needs the training graph (gg_set_graph_csr)");
    GG_CHECK(ctx, deg, GG_EINVAL, "gg_distinct_degrees: deg must not be NULL");
    GG_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = ensure_set_adjacency(ctx);
    if (rc != GG_OK) return rc;
    for (int v = 0; v < ctx->n_node; ++v) deg[v] = (int32_t)(ctx->set.h_ptr[v + 1] - ctx->set.h_ptr[v]);
    return GG_OK;
}

extern "C" int gg_pair_neighbors(gg_ctx *ctx, const int32_t *u, const int32_t *v, int64_t m, const uint64_t *weights, int32_t n_w, int32_t *cn,
                                 int32_t *deg_u, int32_t *deg_v, uint64_t *wsum, double *kernel_ms) {
    const char *fn = "gg_pair_neighbors";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (kernel_ms) *kernel_ms = 0.0;
    GG_CHECK(ctx, ctx->g_rowptr, GG_EINVAL, "%s: needs the training graph (gg_set_graph_csr)", fn);
    GG_CHECK(ctx, n_w >= 0 && n_w <= PN_MAX_W, GG_EINVAL, "%s: n_w = %d outside [0, %d]", fn, n_w, PN_MAX_W);
    GG_CHECK(ctx, m >= 0, GG_EINVAL, "%s: m = %lld is negative", fn, (long long)m);
    if (m == 0) return GG_OK;
    GG_CHECK(ctx, n_w == 0 || (weights && wsum), GG_EINVAL, "%s: weights and wsum must not be NULL when n_w > 0", fn);
    GG_CHECK(ctx, u && v, GG_EINVAL, "%s: u and v must not be NULL", fn);
    GG_CHECK(ctx, cn && deg_u && deg_v, GG_EINVAL, "%s: cn, deg_u and deg_v must not be NULL", fn);
    const int n = ctx->n_node;
    int rc = check_ids(ctx, fn, "u", u, m);
    if (rc == GG_OK) rc = check_ids(ctx, fn, "v", v, m);
    if (rc != GG_OK) return rc;
    GG_HIP(ctx, hipSetDevice(ctx->device));
    rc = ensure_set_adjacency(ctx);
    if (rc == GG_OK) rc = check_weight_bound(ctx, fn, weights, (int64_t)n_w * n);
    if (rc != GG_OK) return rc;

    const int64_t *hp = ctx->set.h_ptr.data();
    const int pass = (int)std::min<int64_t>(m, PN_PASS);
    ScopedBuf d_u, d_v, d_cn, d_du, d_dv, d_ws, d_w, d_task;
    hipError_t e = d_u.reserve(sizeof(int32_t) * pass);
    for (ScopedBuf *b : {&d_v, &d_cn, &d_du, &d_dv})
        if (e == hipSuccess) e = b->reserve(sizeof(int32_t) * pass);
    if (e == hipSuccess && n_w) e = d_ws.reserve(sizeof(uint64_t) * (size_t)n_w * pass);
    if (e == hipSuccess && n_w) e = d_w.reserve(sizeof(uint64_t) * (size_t)n_w * n);
    if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "%s: %s", fn, hipGetErrorString(e));
    if (n_w) GG_HIP_FN(hipMemcpyAsync(d_w.p, weights, sizeof(uint64_t) * (size_t)n_w * n, hipMemcpyHostToDevice, ctx->stream));
    std::vector<int2> task;
    double ms_total = 0.0;
    for (int64_t p0 = 0; p0 < m; p0 += pass) {
        const int cr = (int)std::min<int64_t>(pass, m - p0);
        // the pass's tasks over the pairs' shorter lists, ordered by group width; an empty list has its task too: it stores the outputs
        int64_t first[4];
        const auto shorter = [&](int i) {
            const int a = u[p0 + i], b = v[p0 + i];
            return std::min(hp[a + 1] - hp[a], hp[b + 1] - hp[b]);
        };
        GG_CHECK(ctx, plan_width_tasks(cr, shorter, {8, 64}, PN_CHUNK, true, task, first), GG_EINVAL, "%s: %lld tasks in one pass", fn, (long long)first[3]);
        e = d_task.reserve(sizeof(int2) * task.size());
        if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "%s: %s", fn, hipGetErrorString(e));
        GG_HIP_FN(hipMemcpyAsync(d_u.p, u + p0, sizeof(int32_t) * cr, hipMemcpyHostToDevice, ctx->stream));
        GG_HIP_FN(hipMemcpyAsync(d_v.p, v + p0, sizeof(int32_t) * cr, hipMemcpyHostToDevice, ctx->stream));
        GG_HIP_FN(hipMemcpyAsync(d_task.p, task.data(), sizeof(int2) * task.size(), hipMemcpyHostToDevice, ctx->stream));
        GG_HIP_FN(hipMemsetAsync(d_cn.p, 0, sizeof(int32_t) * cr, ctx->stream));  // (the chunk tasks of the long pairs add)
        if (n_w) GG_HIP_FN(hipMemsetAsync(d_ws.p, 0, sizeof(uint64_t) * (size_t)n_w * cr, ctx->stream));
        PnArgs o{d_u.as<int32_t>(), d_v.as<int32_t>(), cr, nullptr, 0, ctx->set.ptr.as<int64_t>(), ctx->set.adj.as<int32_t>(), d_w.as<uint64_t>(), n_w, n,
                 d_cn.as<int32_t>(), d_du.as<int32_t>(), d_dv.as<int32_t>(), d_ws.as<unsigned long long>()};
        (void)hipEventRecord(ctx->ev0, ctx->stream);
        launch_width_classes(ctx->stream, PN_BLOCKS, d_task.as<int2>(), first, o, pn_sweep_kernel<4>, pn_sweep_kernel<16>, pn_sweep_kernel<64>);
        (void)hipEventRecord(ctx->ev1, ctx->stream);
        GG_HIP_FN(hipGetLastError());
        GG_HIP_FN(hipMemcpyAsync(cn + p0, d_cn.p, sizeof(int32_t) * cr, hipMemcpyDeviceToHost, ctx->stream));
        GG_HIP_FN(hipMemcpyAsync(deg_u + p0, d_du.p, sizeof(int32_t) * cr, hipMemcpyDeviceToHost, ctx->stream));
        GG_HIP_FN(hipMemcpyAsync(deg_v + p0, d_dv.p, sizeof(int32_t) * cr, hipMemcpyDeviceToHost, ctx->stream));
        for (int j = 0; j < n_w; ++j)
            GG_HIP_FN(hipMemcpyAsync(wsum + (int64_t)j * m + p0, d_ws.as<uint64_t>() + (int64_t)j * cr, sizeof(uint64_t) * cr, hipMemcpyDeviceToHost, ctx->stream));
        GG_HIP_FN(hipStreamSynchronize(ctx->stream));
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
        ms_total += ms;
    }
    if (kernel_ms) *kernel_ms = ms_total;
    return GG_OK;
}
