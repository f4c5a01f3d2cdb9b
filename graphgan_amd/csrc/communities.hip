// communities.hip -- the neighbour-mode sweep: every node takes the most frequent label among its neighbours in the resident
// training graph (gg_neighbor_mode), the step of label-propagation community detection (Raghavan et al. 2007), which
// gg_label_propagation iterates on the device; and the intra-community edge counts and degree sums of a partition
// (gg_partition_edges), from which modularity is one float64 formula on the host.  No embedding table is read: integer gathers
// over the SET adjacency of ensure_set_adjacency (pair_neighbors.hip).  The kernels hold no floating-point operation.
//
// Shape (the first build; what was not tuned is listed in DESIGN.md "Neighbour-mode sweep"), by the node's distinct degree d:
//   d <= 64     a group of W = 4, 16 or 64 lanes per node (the smallest that holds the list): each lane gathers one neighbour's
//               label, counts the equal labels of its group by broadcast and compare, and the group folds the triples
//               (count descending, fmix32(l ^ salt) ascending, l ascending) by a shuffle tree;
//   d <= 2048   one workgroup per node counts the labels in a (label, uint32 count) SetTable (set_sweep.h) in LDS
//               (CM_LDS_CAP = 2048 entries -> 4096 slots, 32 KiB: five workgroups share a CU's 160 KiB), then scans the table
//               for the best triple and for the count of the node's own label;
//   d > 2048    the same on a zeroed table in global memory, per task T key words and then T count words of the context's
//               scratch buffer.
// No list is truncated and no path depends on how many distinct labels occur.  Counts are integers and the fold is a total
// order on (count, hash, label), so a node's result depends on its list and the labels alone -- not on the request, the grid,
// the order of the inserts or the run.  The side test of label propagation is an ARGUMENT of the one set of kernels (side_h),
// so T iterations of gg_label_propagation equal 2 T calls of gg_neighbor_mode composed on the host, bit for bit.
#include <algorithm>

#include "set_sweep.h"

namespace gg {

namespace {

constexpr int CM_LDS_CAP = 2048;     // entries of a list the LDS table takes (Engine.NEIGHBOR_MODE_LDS_CAP); longer lists use global memory
constexpr int CM_LDS_SLOTS = 2 * CM_LDS_CAP;
constexpr int CM_CHUNK = 512;        // entries of a node's list per task of gg_partition_edges (Engine.PARTITION_EDGES_CHUNK)
constexpr int CM_BLOCKS = 2048;      // workgroups per launch at most (8 per CU); the groups stride over the tasks behind them
constexpr int CM_CLASSES = 5;        // W = 4, 16, 64, the LDS table, the global table

struct CmArgs {
    const int32_t *task;       // [n_task] request rows of this launch
    int n_task;
    const int64_t *goff;       // global-table launch: [n_task] first word of the task's table in tab
    uint32_t *tab;             //   zeroed: T label words, then T count words per task
    const int32_t *nodes;      // [m] request row -> node, or NULL (the row is the node)
    const int64_t *ptr;        // set adjacency
    const int32_t *adj;
    const int32_t *labels;     // [n_node]
    int32_t *out;              // [m]
    uint32_t salt;
    int keep;
    int side_h;                // -1: every node; 0 / 1: only the nodes with (fmix32(v ^ st) & 1) == side_h, the others copy their label
    uint32_t st;
    unsigned int *changed;     // += the rows whose label moved, or NULL
};

// the fold's order: more neighbours first, then the smaller hash, then the smaller label
__device__ __forceinline__ bool cm_better(uint32_t c1, uint32_t h1, uint32_t l1, uint32_t c2, uint32_t h2, uint32_t l2) {
    return c1 > c2 || (c1 == c2 && (h1 < h2 || (h1 == h2 && l1 < l2)));
}

__device__ __forceinline__ bool cm_mine(const CmArgs &o, int v) { return o.side_h < 0 || (int)(fmix32((uint32_t)v ^ o.st) & 1u) == o.side_h; }

__device__ __forceinline__ void cm_count_changed(unsigned int *changed, unsigned int mine) {
    if (!changed) return;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor(mine, off, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(changed, mine);
}

template <int W>
__global__ __launch_bounds__(256) void cm_mode_group_kernel(CmArgs o) {
    const int gl = threadIdx.x & (W - 1);
    const int groups = gridDim.x * (256 / W);
    unsigned int moved = 0;
    for (int t = blockIdx.x * (256 / W) + threadIdx.x / W; t < o.n_task; t += groups) {  // (the same trip count in every lane of a group)
        const int i = o.task[t];
        const int v = o.nodes ? o.nodes[i] : i;
        const int own = o.labels[v];
        int res = own;
        if (cm_mine(o, v)) {
            const int64_t b0 = o.ptr[v];
            const int d = (int)(o.ptr[v + 1] - b0);  // <= W by the plan
            const int lab = gl < d ? o.labels[o.adj[b0 + gl]] : -1;  // (labels are >= 0: -1 equals none of them)
            uint32_t c = 0, own_c = 0;
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const int x = __shfl(lab, k, W);
                c += x == lab;
                own_c += x == own;
            }
            if (gl >= d) c = 0;
            uint32_t l = (uint32_t)lab, h = fmix32(l ^ o.salt);
#pragma unroll
            for (int off = W / 2; off >= 1; off >>= 1) {
                const uint32_t c2 = __shfl_xor(c, off, W), h2 = __shfl_xor(h, off, W), l2 = __shfl_xor(l, off, W);
                if (cm_better(c2, h2, l2, c, h, l)) c = c2, h = h2, l = l2;
            }
            if (d > 0 && !(o.keep && own_c == c)) res = (int)l;
        }
        if (gl == 0) {
            o.out[i] = res;
            moved += res != own;
        }
    }
    cm_count_changed(o.changed, moved);
}

// one workgroup per node; GLOBAL: the table lies in o.tab (zeroed by the host), else in LDS (zeroed here)
template <bool GLOBAL>
__global__ __launch_bounds__(256) void cm_mode_table_kernel(CmArgs o) {
    __shared__ uint32_t s_key[GLOBAL ? 1 : CM_LDS_SLOTS], s_cnt[GLOBAL ? 1 : CM_LDS_SLOTS];
    __shared__ uint32_t r_c[4], r_h[4], r_l[4], r_own[4];
    const int tid = threadIdx.x;
    for (int t = blockIdx.x; t < o.n_task; t += gridDim.x) {  // (block-uniform: the barriers below are reached by every thread)
        const int i = o.task[t];
        const int v = o.nodes ? o.nodes[i] : i;
        const int own = o.labels[v];
        if (!cm_mine(o, v)) {
            if (tid == 0) o.out[i] = own;
            continue;
        }
        const int64_t b0 = o.ptr[v];
        const int d = (int)(o.ptr[v + 1] - b0);
        const uint32_t T = set_table_slots((uint32_t)d);  // (d <= 2^30 and, on the LDS path, d <= CM_LDS_CAP: T <= CM_LDS_SLOTS)
        SetTable<uint32_t, GLOBAL> tb;  // at most d distinct labels
        tb.key = GLOBAL ? o.tab + o.goff[t] : s_key;
        tb.val = GLOBAL ? tb.key + T : s_cnt;
        tb.mask = T - 1u;
        if (!GLOBAL) tb.clear_lds();
        for (int e = tid; e < d; e += 256) tb.add(o.labels[o.adj[b0 + e]], 1u);
        tb.fill_done();
        uint32_t c = 0, h = 0xffffffffu, l = 0xffffffffu, own_c = 0;
        for (uint32_t s = tid; s < T; s += 256) {
            const uint32_t k = tb.ld_key(s);
            if (k == 0u) continue;
            const uint32_t c2 = tb.ld_val(s);
            const uint32_t l2 = k - 1u, h2 = fmix32(l2 ^ o.salt);
            if (l2 == (uint32_t)own) own_c = c2;
            if (cm_better(c2, h2, l2, c, h, l)) c = c2, h = h2, l = l2;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const uint32_t c2 = __shfl_xor(c, off, 64), h2 = __shfl_xor(h, off, 64), l2 = __shfl_xor(l, off, 64);
            if (cm_better(c2, h2, l2, c, h, l)) c = c2, h = h2, l = l2;
            own_c = max(own_c, __shfl_xor(own_c, off, 64));
        }
        if ((tid & 63) == 0) r_c[tid >> 6] = c, r_h[tid >> 6] = h, r_l[tid >> 6] = l, r_own[tid >> 6] = own_c;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w) {
                if (cm_better(r_c[w], r_h[w], r_l[w], c, h, l)) c = r_c[w], h = r_h[w], l = r_l[w];
                own_c = max(own_c, r_own[w]);
            }
            const int res = (o.keep && own_c == c) ? own : (int)l;
            o.out[i] = res;
            if (o.changed && res != own) atomicAdd(o.changed, 1u);
        }
        __syncthreads();  // (the next task clears the table and the fold words)
    }
}

__global__ __launch_bounds__(256) void cm_iota_kernel(int32_t *L, int n) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n) L[v] = (int32_t)v;
}

struct CeArgs {
    const int2 *task;          // [n_task] (node, first entry)
    int n_task;
    const int64_t *ptr;
    const int32_t *adj;
    const int32_t *assign;     // [n_node] class or -1
    unsigned long long *intra, *tot;  // [n_label], zeroed
};

// Every lane of the wavefront calls this: the lanes with `flag` add (n_in, n_same) into class c, the lanes of one class through
// ONE lane -- a partition of few classes would otherwise send every add of the sweep to the same few addresses.
__device__ __forceinline__ void ce_flush(const CeArgs &o, bool flag, int c, int n_in, int n_same) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(flag);
    while (todo) {  // (todo is the same in every lane)
        const int src = __ffsll((long long)todo) - 1;
        const int cc = __shfl(c, src, 64);
        const bool same = flag && c == cc;
        const unsigned long long mask = __ballot(same);
        int s_in = same ? n_in : 0, s_same = same ? n_same : 0;
        if (mask & (mask - 1)) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                s_in += __shfl_xor(s_in, off, 64);
                s_same += __shfl_xor(s_same, off, 64);
            }
        }
        if (lane == src) {  // integer adds: exact, whatever their order
            atomicAdd(o.tot + cc, (unsigned long long)s_in);
            if (s_same) atomicAdd(o.intra + cc, (unsigned long long)s_same);
        }
        todo &= ~mask;
    }
}

// A group's first lane HOLDS the counts of its tasks while their class stays the same and adds them when it changes or the
// sweep ends.  A wavefront's tasks hold fewer than 2^31 entries (at most 2^31 tasks of at most CM_CHUNK entries over at least
// 8192 / (64 / W) wavefront rounds), so the held counts and their sums over a wavefront fit in an int.
template <int W>
__global__ __launch_bounds__(256) void cm_edges_kernel(CeArgs o) {
    const int gl = threadIdx.x & (W - 1);
    const int groups = gridDim.x * (256 / W);
    int held_c = -1, held_in = 0, held_same = 0;
    for (int base = blockIdx.x * (256 / W); base < o.n_task; base += groups) {  // (the same trip count in every lane of the workgroup)
        const int t = base + threadIdx.x / W;
        int c = -1, n_in = 0, n_same = 0;
        if (t < o.n_task) {
            const int2 tk = o.task[t];
            const int v = tk.x, c0 = tk.y;
            c = o.assign[v];
            if (c >= 0) {  // (else outside the partition)
                const int64_t b0 = o.ptr[v];
                const int end = min((int)(o.ptr[v + 1] - b0), c0 + CM_CHUNK);
                for (int e = c0 + gl; e < end; e += W) {
                    const int a = o.assign[o.adj[b0 + e]];
                    n_in += a >= 0;
                    n_same += a == c;
                }
            }
        }
#pragma unroll
        for (int off = W / 2; off >= 1; off >>= 1) {
            n_in += __shfl_xor(n_in, off, W);
            n_same += __shfl_xor(n_same, off, W);
        }
        const bool has = gl == 0 && n_in > 0, flush = has && held_in > 0 && c != held_c;
        ce_flush(o, flush, held_c, held_in, held_same);
        if (flush) held_in = held_same = 0;
        if (has) held_c = c, held_in += n_in, held_same += n_same;
    }
    ce_flush(o, held_in > 0, held_c, held_in, held_same);
}

int mode_class(int64_t d) { return d <= 4 ? 0 : d <= 16 ? 1 : d <= 64 ? 2 : d <= CM_LDS_CAP ? 3 : 4; }

// The tasks of a neighbour-mode request, ordered by class; the global tables of the giant lists, one per TASK (a repeated node
// has one per occurrence).  (Not set_sweep.h's planner: five classes of whole rows, and the table offsets come out of the fill.)
static_assert(sizeof(DevModePlan::first) == sizeof(int64_t) * (CM_CLASSES + 1), "DevModePlan holds the classes' first tasks");
struct ModePlan {
    std::vector<int32_t> task;
    std::vector<int64_t> goff;
    int64_t first[CM_CLASSES + 1] = {};
    int64_t tab_words = 0;
};

void build_mode_plan(const int64_t *hp, const int32_t *nodes, int64_t m, ModePlan &p) {
    for (int64_t i = 0; i < m; ++i) {
        const int v = nodes ? nodes[i] : (int)i;
        ++p.first[mode_class(hp[v + 1] - hp[v]) + 1];
    }
    for (int c = 0; c < CM_CLASSES; ++c) p.first[c + 1] += p.first[c];
    p.task.resize((size_t)m);
    p.goff.resize((size_t)(p.first[5] - p.first[4]));
    int64_t fill[CM_CLASSES];
    std::copy(p.first, p.first + CM_CLASSES, fill);
    for (int64_t i = 0; i < m; ++i) {
        const int v = nodes ? nodes[i] : (int)i;
        const int64_t d = hp[v + 1] - hp[v];
        const int c = mode_class(d);
        if (c == 4) {
            p.goff[(size_t)(fill[4] - p.first[4])] = p.tab_words;
            p.tab_words += 2 * set_table_slots(d);
        }
        p.task[(size_t)fill[c]++] = (int32_t)i;
    }
}

int upload_mode_plan(gg_ctx *ctx, const char *fn, const ModePlan &p, DevBuf &d_task, DevBuf &d_goff, DevModePlan &dp) {
    hipError_t e = d_task.reserve(sizeof(int32_t) * std::max<size_t>(p.task.size(), 1));
    if (e == hipSuccess) e = d_goff.reserve(sizeof(int64_t) * std::max<size_t>(p.goff.size(), 1));
    if (e == hipSuccess) e = ctx->set.cm_tab.reserve(sizeof(uint32_t) * (size_t)std::max<int64_t>(p.tab_words, 1));
    if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "%s: %s", fn, hipGetErrorString(e));
    if (!p.task.empty()) GG_HIP_FN(hipMemcpyAsync(d_task.p, p.task.data(), sizeof(int32_t) * p.task.size(), hipMemcpyHostToDevice, ctx->stream));
    if (!p.goff.empty()) GG_HIP_FN(hipMemcpyAsync(d_goff.p, p.goff.data(), sizeof(int64_t) * p.goff.size(), hipMemcpyHostToDevice, ctx->stream));
    GG_HIP_FN(hipStreamSynchronize(ctx->stream));  // (the host vectors end with the caller's scope)
    dp.task = d_task.as<int32_t>();
    dp.goff = d_goff.as<int64_t>();
    std::copy(p.first, p.first + CM_CLASSES + 1, dp.first);
    dp.tab_words = p.tab_words;
    return GG_OK;
}

// The all-nodes plans are functions of the graph: built once behind the set adjacency, kept in the context and dropped by
// gg_set_graph_csr (SetGraph::drop): ctx->set.mode, and ctx->set.edges, the (node, first entry) tasks of gg_partition_edges by group
// width (d <= 8 -> 4 lanes, d <= 64 -> 16, else 64) with CM_CHUNK entries per task and none for an empty list.
int ensure_plans(gg_ctx *ctx, const char *fn) {
    const int rc = ensure_set_adjacency(ctx);
    if (rc != GG_OK) return rc;
    SetGraph &g = ctx->set;
    if (g.mode_valid) return GG_OK;
    const int64_t *hp = g.h_ptr.data();
    ModePlan p;
    build_mode_plan(hp, nullptr, ctx->n_node, p);
    const int rc2 = upload_mode_plan(ctx, fn, p, g.cm_task, g.cm_goff, g.mode);
    if (rc2 != GG_OK) return rc2;
    std::vector<int2> et;
    GG_CHECK(ctx, plan_width_tasks(ctx->n_node, [&](int v) { return hp[v + 1] - hp[v]; }, {8, 64}, CM_CHUNK, false, et, g.edges.first), GG_EINVAL,
             "%s: too many tasks", fn);
    const hipError_t e = g.cm_etask.reserve(sizeof(int2) * std::max<size_t>(et.size(), 1));
    if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "%s: %s", fn, hipGetErrorString(e));
    if (!et.empty()) GG_HIP_FN(hipMemcpy(g.cm_etask.p, et.data(), sizeof(int2) * et.size(), hipMemcpyHostToDevice));
    g.edges.task = g.cm_etask.as<int2>();
    g.mode_valid = true;
    return GG_OK;
}

// one sweep: the launches of the five classes (o.task / n_task are set per class)
hipError_t launch_mode(gg_ctx *ctx, CmArgs o, const DevModePlan &dp) {
    if (ctx->set.max_deg > (1 << 30)) return hipErrorInvalidValue;  // (a table of 2 deg slots must stay below 2^32)
    if (dp.tab_words) {
        const hipError_t e = hipMemsetAsync(ctx->set.cm_tab.p, 0, sizeof(uint32_t) * (size_t)dp.tab_words, ctx->stream);
        if (e != hipSuccess) return e;
    }
    o.tab = ctx->set.cm_tab.as<uint32_t>();
    o.goff = dp.goff;
    launch_width_classes(ctx->stream, CM_BLOCKS, dp.task, dp.first, o, cm_mode_group_kernel<4>, cm_mode_group_kernel<16>, cm_mode_group_kernel<64>);
    for (int c = 3; c < CM_CLASSES; ++c) {  // the table kernels: one workgroup per task
        const int64_t n_task = dp.first[c + 1] - dp.first[c];
        if (n_task == 0) continue;
        o.task = dp.task + dp.first[c];
        o.n_task = (int)n_task;
        const dim3 grid((unsigned)std::min<int64_t>(CM_BLOCKS, n_task)), block(256);
        if (c == 3) hipLaunchKernelGGL(cm_mode_table_kernel<false>, grid, block, 0, ctx->stream, o);
        else hipLaunchKernelGGL(cm_mode_table_kernel<true>, grid, block, 0, ctx->stream, o);
    }
    return hipGetLastError();
}

}  // namespace

}  // namespace gg

using namespace gg;

// gg_neighbor_mode, gg_label_propagation, gg_partition_edges: see include/graphgan_hip.h.
extern "C" int gg_neighbor_mode(gg_ctx *ctx, const int32_t *labels, uint32_t salt, int32_t keep, const int32_t *nodes, int64_t m, int32_t *out,
                                double *kernel_ms) {
    const char *fn = "gg_neighbor_mode";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (kernel_ms) *kernel_ms = 0.0;
    GG_CHECK(ctx, ctx->g_rowptr, GG_EINVAL, "%s: needs the training graph (gg_set_graph_csr)", fn);
    const int n = ctx->n_node;
    if (!nodes) m = n;
    GG_CHECK(ctx, m >= 0, GG_EINVAL, "%s: m = %lld is negative", fn, (long long)m);
    if (m == 0) return GG_OK;
    GG_CHECK(ctx, labels && out, GG_EINVAL, "%s: labels and out must not be NULL", fn);
    GG_CHECK(ctx, m <= 0x7fffffffLL, GG_EINVAL, "%s: m = %lld does not fit in 31 bits", fn, (long long)m);
    for (int v = 0; v < n; ++v) GG_CHECK(ctx, labels[v] >= 0, GG_EINVAL, "%s: labels[%d] = %d is negative", fn, v, labels[v]);
    if (nodes) {
        const int rc = check_ids(ctx, fn, "nodes", nodes, m);
        if (rc != GG_OK) return rc;
    }
    GG_HIP(ctx, hipSetDevice(ctx->device));
    DevModePlan own;  // the plan of a request of some nodes
    ScopedBuf d_task, d_goff;
    if (nodes) {
        const int rc = ensure_set_adjacency(ctx);
        if (rc != GG_OK) return rc;
        ModePlan p;
        build_mode_plan(ctx->set.h_ptr.data(), nodes, m, p);
        const int rc2 = upload_mode_plan(ctx, fn, p, d_task, d_goff, own);
        if (rc2 != GG_OK) return rc2;
    } else {
        const int rc = ensure_plans(ctx, fn);
        if (rc != GG_OK) return rc;
    }
    const DevModePlan &dp = nodes ? own : ctx->set.mode;
    ScopedBuf d_lab, d_out, d_nodes;
    hipError_t e = d_lab.reserve(sizeof(int32_t) * (size_t)n);
    if (e == hipSuccess) e = d_out.reserve(sizeof(int32_t) * (size_t)m);
    if (e == hipSuccess && nodes) e = d_nodes.reserve(sizeof(int32_t) * (size_t)m);
    if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "%s: %s", fn, hipGetErrorString(e));
    GG_HIP_FN(hipMemcpyAsync(d_lab.p, labels, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    if (nodes) GG_HIP_FN(hipMemcpyAsync(d_nodes.p, nodes, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    CmArgs o{};
    o.nodes = nodes ? d_nodes.as<int32_t>() : nullptr;
    o.ptr = ctx->set.ptr.as<int64_t>();
    o.adj = ctx->set.adj.as<int32_t>();
    o.labels = d_lab.as<int32_t>();
    o.out = d_out.as<int32_t>();
    o.salt = salt;
    o.keep = keep != 0;
    o.side_h = -1;
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    GG_HIP_FN(launch_mode(ctx, o, dp));
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    GG_HIP_FN(hipMemcpyAsync(out, d_out.p, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    if (kernel_ms) *kernel_ms = ms;
    return GG_OK;
}

extern "C" int gg_label_propagation(gg_ctx *ctx, uint32_t seed, int32_t max_iters, int32_t *labels, int32_t *iters, int32_t *converged, int32_t *changed,
                                    double *kernel_ms) {
    const char *fn = "gg_label_propagation";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (kernel_ms) *kernel_ms = 0.0;
    GG_CHECK(ctx, ctx->g_rowptr, GG_EINVAL, "%s: needs the training graph (gg_set_graph_csr)", fn);
    GG_CHECK(ctx, max_iters >= 1, GG_EINVAL, "%s: max_iters = %d is below 1", fn, max_iters);
    GG_CHECK(ctx, labels && iters && converged && changed, GG_EINVAL, "%s: labels, iters, converged and changed must not be NULL", fn);
    const int n = ctx->n_node;
    GG_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = ensure_plans(ctx, fn);
    if (rc != GG_OK) return rc;
    const DevModePlan &dp = ctx->set.mode;
    // the state lives on the device for the whole call: L before and behind a half-step (ping-pong) and one changed word per iteration
    ScopedBuf d_L[2], d_changed;
    hipError_t e = d_L[0].reserve(sizeof(int32_t) * (size_t)std::max(n, 1));
    if (e == hipSuccess) e = d_L[1].reserve(sizeof(int32_t) * (size_t)std::max(n, 1));
    if (e == hipSuccess) e = d_changed.reserve(sizeof(unsigned int) * (size_t)max_iters);
    if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "%s: %s", fn, hipGetErrorString(e));
    GG_HIP_FN(hipMemsetAsync(d_changed.p, 0, sizeof(unsigned int) * (size_t)max_iters, ctx->stream));
    CmArgs o{};
    o.ptr = ctx->set.ptr.as<int64_t>();
    o.adj = ctx->set.adj.as<int32_t>();
    o.keep = 1;
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    if (n) hipLaunchKernelGGL(cm_iota_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, d_L[0].as<int32_t>(), n);
    int t = 0, done = 0;
    while (t < max_iters && !done) {
        ++t;
        o.st = fmix32((seed ^ 0x85ebca6bu) + 0x9E3779B9u * (uint32_t)t);
        o.changed = d_changed.as<unsigned int>() + (t - 1);
        for (int h = 0; h < 2; ++h) {  // L[0] -> L[1] -> L[0]: an iteration ends where it began
            o.labels = d_L[h].as<int32_t>();
            o.out = d_L[h ^ 1].as<int32_t>();
            o.salt = fmix32(seed + 0x9E3779B9u * (uint32_t)(2 * (t - 1) + h + 1));
            o.side_h = h;
            GG_HIP_FN(launch_mode(ctx, o, dp));
        }
        unsigned int moved = 0;  // the one word that crosses to the host per iteration
        GG_HIP_FN(hipMemcpyAsync(&moved, o.changed, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
        GG_HIP_FN(hipStreamSynchronize(ctx->stream));
        changed[t - 1] = (int32_t)moved;
        done = moved == 0;
    }
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    if (n) GG_HIP_FN(hipMemcpyAsync(labels, d_L[0].p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipStreamSynchronize(ctx->stream));
    *iters = t;
    *converged = done;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    if (kernel_ms) *kernel_ms = ms;
    return GG_OK;
}

extern "C" int gg_partition_edges(gg_ctx *ctx, const int32_t *assign, int32_t n_label, int64_t *intra, int64_t *tot, double *kernel_ms) {
    const char *fn = "gg_partition_edges";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (kernel_ms) *kernel_ms = 0.0;
    GG_CHECK(ctx, ctx->g_rowptr, GG_EINVAL, "%s: needs the training graph (gg_set_graph_csr)", fn);
    GG_CHECK(ctx, n_label >= 1, GG_EINVAL, "%s: n_label = %d is below 1", fn, n_label);
    GG_CHECK(ctx, assign && intra && tot, GG_EINVAL, "%s: assign, intra and tot must not be NULL", fn);
    const int n = ctx->n_node;
    for (int v = 0; v < n; ++v)
        GG_CHECK(ctx, assign[v] >= -1 && assign[v] < n_label, GG_EINVAL, "%s: assign[%d] = %d outside [-1, %d)", fn, v, assign[v], n_label);
    GG_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = ensure_plans(ctx, fn);
    if (rc != GG_OK) return rc;
    ScopedBuf d_assign, d_cnt;
    hipError_t e = d_assign.reserve(sizeof(int32_t) * (size_t)std::max(n, 1));
    if (e == hipSuccess) e = d_cnt.reserve(sizeof(int64_t) * 2 * (size_t)n_label);
    if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "%s: %s", fn, hipGetErrorString(e));
    if (n) GG_HIP_FN(hipMemcpyAsync(d_assign.p, assign, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    GG_HIP_FN(hipMemsetAsync(d_cnt.p, 0, sizeof(int64_t) * 2 * (size_t)n_label, ctx->stream));
    CeArgs o{};
    o.ptr = ctx->set.ptr.as<int64_t>();
    o.adj = ctx->set.adj.as<int32_t>();
    o.assign = d_assign.as<int32_t>();
    o.intra = d_cnt.as<unsigned long long>();
    o.tot = o.intra + n_label;
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    launch_width_classes(ctx->stream, CM_BLOCKS, ctx->set.edges.task, ctx->set.edges.first, o, cm_edges_kernel<4>, cm_edges_kernel<16>, cm_edges_kernel<64>);
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    GG_HIP_FN(hipGetLastError());
    GG_HIP_FN(hipMemcpyAsync(intra, d_cnt.p, sizeof(int64_t) * (size_t)n_label, hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipMemcpyAsync(tot, d_cnt.as<int64_t>() + n_label, sizeof(int64_t) * (size_t)n_label, hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    if (kernel_ms) *kernel_ms = ms;
    return GG_OK;
}
