// spanning_forest.hip -- the undirected edge list of the resident training graph (gg_undirected_edges) and its minimum spanning
// forest under distinct 64-bit keys with the connected components (gg_spanning_forest): Boruvka rounds over the resident edge
// list.  No embedding table is read: integer gathers over the SET adjacency of ensure_set_adjacency (pair_neighbors.hip).  The
// kernels hold no floating-point operation.
//
// Shape (the first build; what was not tuned is listed in DESIGN.md "Spanning-forest sweep").  comp[v] names the root of v's
// current component, parent[] is comp at the start of a round.  A round is two sweeps of one thread per edge:
//   sf_min    an edge between two components asks for best[c] = min(best[c], key) on both; the lanes of a wavefront that ask for
//             the same component one behind the other ask once, and an ask that cannot lower best[c] (a relaxed load) is dropped;
//   sf_hook   the edge whose key is best[c] joins c to the component at its other end: parent[c] = other; two components that
//             chose each other (the one cycle distinct keys allow) are joined once, the larger root under the smaller.
// Then parent <- parent[parent] a fixed number of times (ceil(log2(components)) + 1 launches: a round may hook a chain as long as
// the graph) and comp[v] = parent[comp[v]].  One 4-byte hook count crosses to the host per round; the loop ends at the first
// round that hooks nothing.  Nothing on the device loops on a condition.  A minimum spanning forest under distinct keys is
// unique, so the result depends on the graph and the keys alone -- not on the grid, the order of the atomics or the run.
#include <algorithm>

#include "set_sweep.h"

namespace gg {

namespace {

constexpr uint32_t SF_SEED_SALT = 0x53504C54u;  // the default priorities: fmix32(j ^ fmix32(seed ^ SF_SEED_SALT))
constexpr unsigned long long SF_NONE = ~0ull;   // no key: every key is smaller (the edge index in its low word is below 2^31)

struct SfArgs {
    const int2 *edge;          // [m] (a, b), a < b, ascending
    int64_t m;
    const uint32_t *prio;      // [m] or NULL: the default priorities of `salt`
    uint32_t salt;             // fmix32(seed ^ SF_SEED_SALT)
    const int32_t *comp;       // [n_node]
    int32_t *parent;           // [n_node]
    unsigned long long *best;  // [n_node]
    uint8_t *forest;           // [m]
    unsigned int *cnt;         // this sweep's words: the parents written (hooks), the edges between two components (live)
};

__device__ __forceinline__ unsigned long long sf_key(const SfArgs &o, int64_t j) {
    const uint32_t p = o.prio ? o.prio[j] : fmix32((uint32_t)j ^ o.salt);
    return ((unsigned long long)p << 32) | (unsigned long long)j;
}

// Every lane of the wavefront calls this; a lane with c >= 0 asks for best[c] = min(best[c], key).  The lanes of a run of equal
// c among consecutive lanes fold their keys by a segmented scan and the run's last lane asks once; the ask is dropped where
// best[c] is already at or below the key (best only ever decreases within a sweep, so a stale read only costs an atomic).
__device__ __forceinline__ void sf_ask_min(unsigned long long *best, int c, unsigned long long key) {
    const int lane = threadIdx.x & 63;
    const int before = __shfl_up(c, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || before != c);  // (bit 0 is always set)
    const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));  // the first lane of this lane's run
    uint32_t lo = (uint32_t)key, hi = (uint32_t)(key >> 32);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t lo2 = __shfl_up(lo, off, 64), hi2 = __shfl_up(hi, off, 64);
        if (lane - off >= start && (hi2 < hi || (hi2 == hi && lo2 < lo))) lo = lo2, hi = hi2;
    }
    const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
    if (c >= 0 && last) {
        key = ((unsigned long long)hi << 32) | lo;
        if (__hip_atomic_load(best + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(best + c, key);
    }
}

__global__ __launch_bounds__(256) void sf_iota_kernel(int32_t *comp, int32_t *parent, int32_t *minid, int n) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n) comp[v] = parent[v] = minid[v] = (int32_t)v;
}

__global__ __launch_bounds__(256) void sf_min_kernel(SfArgs o) {
    __shared__ unsigned int s_live;
    if (threadIdx.x == 0) s_live = 0u;
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int cu = -1, cv = -1;  // (-1: nothing to ask)
    unsigned long long key = SF_NONE;
    if (j < o.m) {
        const int2 e = o.edge[j];
        const int x = o.comp[e.x], y = o.comp[e.y];
        if (x != y) cu = x, cv = y, key = sf_key(o, j);
    }
    sf_ask_min(o.best, cu, key);
    sf_ask_min(o.best, cv, key);
    const unsigned long long live = __ballot(cu >= 0);
    if ((threadIdx.x & 63) == 0 && live) atomicAdd(&s_live, (unsigned int)__popcll(live));
    __syncthreads();
    if (threadIdx.x == 0 && s_live) atomicAdd(o.cnt + 1, s_live);
}

__global__ __launch_bounds__(256) void sf_hook_kernel(SfArgs o) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool hook = false;
    if (j < o.m) {
        const int2 e = o.edge[j];
        const int cu = o.comp[e.x], cv = o.comp[e.y];
        if (cu != cv) {
            const unsigned long long key = sf_key(o, j);
            const bool wu = o.best[cu] == key, wv = o.best[cv] == key;
            hook = wu || wv;
            if (hook) {  // (each root is the target of exactly one such edge: keys are distinct)
                o.forest[j] = 1;
                if (wu && wv) o.parent[max(cu, cv)] = min(cu, cv);
                else if (wu) o.parent[cu] = cv;
                else o.parent[cv] = cu;
            }
        }
    }
    const unsigned long long hooks = __ballot(hook);
    if ((threadIdx.x & 63) == 0 && hooks) atomicAdd(o.cnt, (unsigned int)__popcll(hooks));
}

__global__ __launch_bounds__(256) void sf_jump_kernel(const int32_t *src, int32_t *dst, int n) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n) dst[v] = src[src[v]];
}

__global__ __launch_bounds__(256) void sf_comp_kernel(const int32_t *parent, int32_t *comp, int n) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n) comp[v] = parent[comp[v]];
}

__global__ __launch_bounds__(256) void sf_minid_kernel(const int32_t *comp, int32_t *minid, int n) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n) {
        const int c = comp[v];
        if (v < c) atomicMin(minid + c, (int)v);  // (minid[c] starts at c, a member of its own component)
    }
}

__global__ __launch_bounds__(256) void sf_label_kernel(const int32_t *comp, const int32_t *minid, int32_t *out, int n) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n) out[v] = minid[comp[v]];
}

int ceil_log2(int64_t x) {  // the smallest k with 2^k >= x, x >= 1
    int k = 0;
    while (((int64_t)1 << k) < x) ++k;
    return k;
}

// the part of a's sorted list behind a: the b of the undirected edges (a, b), a < b (behind ensure_set_adjacency)
struct UpperList {
    const int32_t *begin, *end;
};
UpperList upper_list(const SetGraph &g, int a) {
    const int32_t *lo = g.h_adj.data() + g.h_ptr[a], *hi = g.h_adj.data() + g.h_ptr[a + 1];
    return {std::upper_bound(lo, hi, a), hi};
}

// The undirected edge list of the resident graph, a function of the graph alone: built once behind the set adjacency, kept in the
// context and dropped by gg_set_graph_csr (SetGraph::drop).
int ensure_undirected_edges(gg_ctx *ctx, const char *fn) {
    const int rc = ensure_set_adjacency(ctx);
    if (rc != GG_OK) return rc;
    SetGraph &g = ctx->set;
    if (g.und_valid) return GG_OK;
    const int n = ctx->n_node;
    int64_t m = 0;
    for (int v = 0; v < n; ++v) {
        const UpperList u = upper_list(g, v);
        m += u.end - u.begin;
    }
    GG_CHECK(ctx, m <= 0x7fffffffLL, GG_EINVAL, "%s: the graph has %lld undirected edges, more than 2^31 - 1", fn, (long long)m);
    std::vector<int2> e((size_t)m);
    size_t at = 0;
    for (int v = 0; v < n; ++v) {
        const UpperList u = upper_list(g, v);
        for (const int32_t *w = u.begin; w < u.end; ++w) e[at++] = make_int2(v, *w);
    }
    hipError_t err = g.und.reserve(sizeof(int2) * std::max<size_t>(e.size(), 1));
    if (err == hipSuccess && m) err = hipMemcpy(g.und.p, e.data(), sizeof(int2) * e.size(), hipMemcpyHostToDevice);
    if (err != hipSuccess) return fail(ctx, GG_ENOMEM, "%s: undirected edge list (%lld edges): %s", fn, (long long)m, hipGetErrorString(err));
    g.und_m = m;
    g.und_valid = true;
    return GG_OK;
}

}  // namespace

}  // namespace gg

using namespace gg;

// gg_undirected_edges, gg_spanning_forest: see include/graphgan_hip.h.
extern "C" int gg_undirected_edges(gg_ctx *ctx, int64_t *m, int32_t *edges) {
    const char *fn = "gg_undirected_edges";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    GG_CHECK(ctx, ctx->g_rowptr, GG_EINVAL, "%s: needs the training graph (gg_set_graph_csr)", fn);
    GG_CHECK(ctx, m, GG_EINVAL, "%s: m must not be NULL", fn);
    GG_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = ensure_undirected_edges(ctx, fn);
    if (rc != GG_OK) return rc;
    *m = ctx->set.und_m;
    if (!edges) return GG_OK;
    int64_t at = 0;
    for (int v = 0; v < ctx->n_node; ++v) {
        const UpperList u = upper_list(ctx->set, v);
        for (const int32_t *w = u.begin; w < u.end; ++w, ++at) edges[2 * at] = v, edges[2 * at + 1] = *w;
    }
    return GG_OK;
}

extern "C" int gg_spanning_forest(gg_ctx *ctx, uint32_t seed, const uint32_t *prio, int64_t n_prio, uint8_t *forest, int32_t *component, int64_t *stats,
                                  int64_t *sweep_counts, double *sweep_ms, double *kernel_ms) {
    const char *fn = "gg_spanning_forest";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (kernel_ms) *kernel_ms = 0.0;
    GG_CHECK(ctx, ctx->g_rowptr, GG_EINVAL, "%s: needs the training graph (gg_set_graph_csr)", fn);
    GG_CHECK(ctx, stats, GG_EINVAL, "%s: stats must not be NULL", fn);
    GG_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = ensure_undirected_edges(ctx, fn);
    if (rc != GG_OK) return rc;
    SetGraph &g = ctx->set;
    const int n = ctx->n_node;
    const int64_t m = g.und_m;
    GG_CHECK(ctx, !prio || n_prio == m, GG_EINVAL, "%s: priority has %lld entries, the graph has %lld undirected edges", fn, (long long)n_prio, (long long)m);
    const int max_rounds = ceil_log2(std::max(n, 2)) + 1;  // every round at least halves the components that still have an outgoing edge
    static_assert(GG_SF_MAX_SWEEPS >= 31 + 1 + 1, "a sweep per round of a graph of 2^31 - 1 nodes and the one that hooks nothing");
    const size_t nn = (size_t)std::max(n, 1), mm = (size_t)std::max<int64_t>(m, 1);
    hipError_t e = g.sf_comp.reserve(sizeof(int32_t) * nn);
    for (DevBuf *b : {&g.sf_parent[0], &g.sf_parent[1], &g.sf_minid})
        if (e == hipSuccess) e = b->reserve(sizeof(int32_t) * nn);
    if (e == hipSuccess) e = g.sf_best.reserve(sizeof(unsigned long long) * nn);
    if (e == hipSuccess) e = g.sf_forest.reserve(mm);
    if (e == hipSuccess) e = g.sf_cnt.reserve(sizeof(unsigned int) * 2 * GG_SF_MAX_SWEEPS);
    ScopedBuf d_prio;
    if (e == hipSuccess && prio) e = d_prio.reserve(sizeof(uint32_t) * mm);
    if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "%s: %s", fn, hipGetErrorString(e));
    if (prio && m) GG_HIP_FN(hipMemcpyAsync(d_prio.p, prio, sizeof(uint32_t) * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    GG_HIP_FN(hipMemsetAsync(g.sf_cnt.p, 0, sizeof(unsigned int) * 2 * GG_SF_MAX_SWEEPS, ctx->stream));
    GG_HIP_FN(hipMemsetAsync(g.sf_forest.p, 0, mm, ctx->stream));
    // per-sweep event pairs only where the caller asks for the times
    std::vector<hipEvent_t> ev;
    struct EvGuard {
        std::vector<hipEvent_t> &v;
        ~EvGuard() { for (hipEvent_t x : v) (void)hipEventDestroy(x); }
    } ev_guard{ev};
    SfArgs o{};
    o.edge = g.und.as<int2>();
    o.m = m;
    o.prio = prio ? d_prio.as<uint32_t>() : nullptr;
    o.salt = fmix32(seed ^ SF_SEED_SALT);
    o.comp = g.sf_comp.as<int32_t>();
    o.best = g.sf_best.as<unsigned long long>();
    o.forest = g.sf_forest.as<uint8_t>();
    const dim3 node_grid((unsigned)cdiv(n, 256)), edge_grid((unsigned)cdiv(m, 256)), block(256);
    int cur = 0;  // sf_parent[cur] equals comp at the start of a round
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    if (n) hipLaunchKernelGGL(sf_iota_kernel, node_grid, block, 0, ctx->stream, g.sf_comp.as<int32_t>(), g.sf_parent[0].as<int32_t>(), g.sf_minid.as<int32_t>(), n);
    int rounds = 0, sweeps = 0;
    int64_t n_forest = 0;
    unsigned int hooks[GG_SF_MAX_SWEEPS] = {};
    while (m > 0) {
        GG_CHECK(ctx, rounds <= max_rounds && sweeps < GG_SF_MAX_SWEEPS, GG_ECAPACITY, "%s: internal error: more than %d rounds on %d nodes", fn, max_rounds, n);
        o.parent = g.sf_parent[cur].as<int32_t>();
        o.cnt = g.sf_cnt.as<unsigned int>() + 2 * sweeps;
        if (sweep_ms) {
            for (int k = 0; k < 2; ++k) {
                hipEvent_t x;
                GG_HIP_FN(hipEventCreate(&x));
                ev.push_back(x);
            }
            (void)hipEventRecord(ev[2 * sweeps], ctx->stream);
        }
        GG_HIP_FN(hipMemsetAsync(g.sf_best.p, 0xff, sizeof(unsigned long long) * nn, ctx->stream));
        hipLaunchKernelGGL(sf_min_kernel, edge_grid, block, 0, ctx->stream, o);
        hipLaunchKernelGGL(sf_hook_kernel, edge_grid, block, 0, ctx->stream, o);
        GG_HIP_FN(hipGetLastError());
        // the one word that crosses to the host per round
        GG_HIP_FN(hipMemcpyAsync(&hooks[sweeps], o.cnt, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
        GG_HIP_FN(hipStreamSynchronize(ctx->stream));
        const unsigned int h = hooks[sweeps];
        if (h) {
            const int jumps = ceil_log2(std::max<int64_t>((int64_t)n - n_forest, 2)) + 1;  // a chain holds at most the components of the round's start
            for (int k = 0; k < jumps; ++k, cur ^= 1)
                hipLaunchKernelGGL(sf_jump_kernel, node_grid, block, 0, ctx->stream, g.sf_parent[cur].as<int32_t>(), g.sf_parent[cur ^ 1].as<int32_t>(), n);
            hipLaunchKernelGGL(sf_comp_kernel, node_grid, block, 0, ctx->stream, g.sf_parent[cur].as<int32_t>(), g.sf_comp.as<int32_t>(), n);
            GG_HIP_FN(hipGetLastError());
        }
        if (sweep_ms) (void)hipEventRecord(ev[2 * sweeps + 1], ctx->stream);
        ++sweeps;
        if (!h) break;
        ++rounds;
        n_forest += h;
    }
    if (n && component) {
        hipLaunchKernelGGL(sf_minid_kernel, node_grid, block, 0, ctx->stream, g.sf_comp.as<int32_t>(), g.sf_minid.as<int32_t>(), n);
        // (the labels are staged in the hook pointers' other buffer, which nothing reads any more)
        hipLaunchKernelGGL(sf_label_kernel, node_grid, block, 0, ctx->stream, g.sf_comp.as<int32_t>(), g.sf_minid.as<int32_t>(), g.sf_parent[cur ^ 1].as<int32_t>(), n);
        GG_HIP_FN(hipGetLastError());
    }
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    if (n && component) GG_HIP_FN(hipMemcpyAsync(component, g.sf_parent[cur ^ 1].p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (m && forest) GG_HIP_FN(hipMemcpyAsync(forest, g.sf_forest.p, (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<unsigned int> cnt(2 * GG_SF_MAX_SWEEPS, 0u);
    if (sweep_counts) GG_HIP_FN(hipMemcpyAsync(cnt.data(), g.sf_cnt.p, sizeof(unsigned int) * cnt.size(), hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipStreamSynchronize(ctx->stream));
    stats[0] = m;
    stats[1] = n_forest;
    stats[2] = (int64_t)n - n_forest;
    stats[3] = rounds;
    for (int s = 0; s < GG_SF_MAX_SWEEPS; ++s) {
        if (sweep_counts) sweep_counts[2 * s] = s < sweeps ? (int64_t)cnt[2 * s + 1] : -1, sweep_counts[2 * s + 1] = s < sweeps ? (int64_t)cnt[2 * s] : -1;
        if (sweep_ms) {
            float ms = 0.f;
            if (s < sweeps) (void)hipEventElapsedTime(&ms, ev[2 * s], ev[2 * s + 1]);
            sweep_ms[s] = s < sweeps ? ms : -1.0;
        }
    }
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    if (kernel_ms) *kernel_ms = ms;
    return GG_OK;
}
