// graph_softmax.hip -- the generator's graph softmax G(v | root) written down exactly: the law of ONE walk of gg_walk_sample
// (reference GraphGAN.sample, src/GraphGAN/graph_gan.py:225-270) on the resident BFS trees, without sampling.
//
// A walk at tree node v draws from the softmax of s(v, w) = g_v . g_w + b_w (generator.py:21) over v's candidate list N(v):
// the children at the root, father + children elsewhere (the father dropped where the D-mode rules or the Q3 bits of
// :256-259 drop it); it steps down to a child or stops, with v as its sample, where it draws its father.  So
//     reach(root) = 1,  reach(c) = reach(v) q(c | v),  P(v) = reach(v) q(father | v),  A = sum of reach over nodes with N(v) empty
// and sum_v P(v) + A = 1 (A: the walk's ``return None, None``).  Everything is computed in log space in float64.
//
// Scores: a private copy of the edge scores es[e] = s(u, col[e]) of every graph edge in float64 from the fp32 tables (the walk
// sampler's layout of spec S1 -- 16-lane groups, float4 chunks, one fma chain per lane, xor butterfly, + bias -- with float64
// fma), filled once per generator state (generator_changed drops it).  float64 and not the walks' fp32 scores: at |s| ~ 10 the
// fp32 rounding of a score moves a probability by ~1e-6 relative, more than the contract's tolerance for A.  The walk sampler's
// own cache and its stamps are never touched, so walks before and after a call are the same walks.  After the fill every
// per-rank access is one gather of a score (8 bytes; one 64-byte sector either way):
//     s(v, child c) = es[t_edge[c]]            (the edge father -> c the BFS appended c at)
//     s(v, father)  = es[g_rev[t_edge[v]]]      (its reverse edge, in v's adjacency)
// Sweep: levels are contiguous rank ranges (level L+1 = [cstart[a_L], cstart[a_{L+1}])), so a parent-driven pass needs no
// father array.  One launch per depth covers that level of every slot of the pass: a thread per rank (lists of <= GS_LONG
// children), a workgroup per rank for longer lists (hubs), queued by the thread that met them.  Each rank computes max and
// log-sum-exp of its candidates and writes logR of its children and log P of itself, scattered by node id into the pass's
// dense rows.  Sums run in a fixed order (per thread in list order; per workgroup strided partials + a fixed LDS tree), no
// floating-point atomics: results do not depend on the other slots of the call, their order or the pass boundaries.
#include <math.h>

#include <algorithm>
#include <vector>

#include "gg_internal.h"

namespace gg {
namespace {

constexpr int GS_LONG = 32;                      // children lists longer than this go to a workgroup (gs_long_kernel)
constexpr int GS_MAX_SLOTS = 4096;               // slots per pass
constexpr size_t GS_DENSE_BYTES = 256ull << 20;  // dense log-probability rows of one pass

struct GsTree {
    const int32_t *t_root, *t_order, *t_cstart, *t_edge;
    const int64_t *t_base;
    const uint32_t *q3;      // removed-father bits (Q3); nullptr = none
    const int64_t *q3off;    // word offset of slot r's row: q3off[q3_by_node ? t_root[r] : r]
    int32_t q3_by_node;      // 1: the persistent store of gg_epoch_* (rows by root node), 0: the slots' own rows
    const int32_t *g_rev;
    const double *es;        // private edge scores (gs_es)
    int32_t for_d;
};

struct GsPass {
    const int32_t *slots;    // [P]
    int32_t P;
    const int64_t *lbase;    // [P + 1] first logR entry of each slot (rank i of slot k at lbase[k] + i)
    double *logR;
    int32_t *lev;            // [P * LW] first rank of level L of slot k at lev[k * LW + L]
    int32_t LW;
    float *dense;            // [P * n_node] log P by node id
    int32_t n_node;
    int2 *long_list;         // (slot of the pass, rank) of the lists of the level that need a workgroup
    int32_t *long_cnt;       // [LW] entries queued per level
};

// is the father entry in N(v) for rank i (> 0) at level L?  (D-mode: the father of a depth-1 node is the root, :256-259;
// Q3: D-mode walks of earlier calls removed it from the lists of depth-1 nodes for good, :258-259)
__device__ __forceinline__ bool father_in(const GsTree &t, int r, int i, int L) {
    if (i == 0) return false;
    if (L != 1) return true;
    if (t.for_d) return false;
    if (!t.q3) return true;
    const int64_t row = t.q3off[t.q3_by_node ? t.t_root[r] : r];
    return !((t.q3[row + ((i - 1) >> 5)] >> ((i - 1) & 31)) & 1u);
}

__device__ __forceinline__ int find_slot(const int64_t *off, int P, int64_t j) {  // last k with off[k] <= j
    int lo = 0, hi = P;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
}

// the edge-score fill: one 16-lane group per 16 consecutive edges of one node's list (chunk c of node u: cpre[u] <= c < cpre[u + 1])
template <int NCH>
__global__ __launch_bounds__(256) void gs_fill_kernel(const float *E, const float *bias, int32_t ld, int32_t nchunk, const int64_t *rowptr,
                                                      const int32_t *col, const int64_t *cpre, int32_t n_node, int64_t n_chunks, double *es) {
    constexpr int UNROLL = 4;
    const int t = threadIdx.x & 15;
    const int64_t n_groups = (int64_t)gridDim.x * 16;
    for (int64_t c = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); c < n_chunks; c += n_groups) {
        const int u = find_slot(cpre, n_node, c);
        const int64_t e0 = rowptr[u] + (c - cpre[u]) * 16;
        const int nb = (int)min((int64_t)16, rowptr[u + 1] - e0);
        float4 gc[NCH];
        const float4 *const crow = (const float4 *)(E + (int64_t)u * ld);
#pragma unroll
        for (int cc = 0; cc < NCH; ++cc) {
            const int ch = t + 16 * cc;
            gc[cc] = (ch < nchunk) ? crow[ch] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const int myid = (t < nb) ? col[e0 + t] : -1;
        const double mybias = (t < nb) ? (double)bias[myid] : 0.0;
        double mysc = 0.0;
        for (int j0 = 0; j0 < nb; j0 += UNROLL) {
            float4 y[UNROLL][NCH];
#pragma unroll
            for (int u2 = 0; u2 < UNROLL; ++u2) {
                const int id = __shfl(myid, j0 + u2, 16);
                const bool valid = id >= 0;
                const float4 *const row = (const float4 *)(E + (int64_t)(valid ? id : 0) * ld);
#pragma unroll
                for (int cc = 0; cc < NCH; ++cc) {
                    const int ch = t + 16 * cc;
                    y[u2][cc] = (valid && ch < nchunk) ? row[ch] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
#pragma unroll
            for (int u2 = 0; u2 < UNROLL; ++u2) {
                double acc = 0.0;
#pragma unroll
                for (int cc = 0; cc < NCH; ++cc) {
                    acc = __builtin_fma((double)gc[cc].x, (double)y[u2][cc].x, acc);
                    acc = __builtin_fma((double)gc[cc].y, (double)y[u2][cc].y, acc);
                    acc = __builtin_fma((double)gc[cc].z, (double)y[u2][cc].z, acc);
                    acc = __builtin_fma((double)gc[cc].w, (double)y[u2][cc].w, acc);
                }
                // xor butterfly over the 16 lanes
                acc += __shfl_xor(acc, 8, 16);
                acc += __shfl_xor(acc, 4, 16);
                acc += __shfl_xor(acc, 2, 16);
                acc += __shfl_xor(acc, 1, 16);
                if (t == j0 + u2) mysc = acc + mybias;
            }
        }
        if (t < nb) es[e0 + t] = mysc;
    }
}

__global__ __launch_bounds__(256) void gs_fill_dense_kernel(float *dense, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dense[i] = -INFINITY;
}

// one thread per slot of the pass: the first rank of every level (a_0 = 0, a_{L+1} = cstart[a_L]); *bad = 1 when the slot's
// segment is not the size the host expects or its levels do not end within LW - 1 of them
__global__ __launch_bounds__(64) void gs_plan_kernel(GsTree t, GsPass p, int32_t *bad) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= p.P) return;
    const int r = p.slots[k];
    const int64_t b = t.t_base[r];
    const int64_t C = p.lbase[k + 1] - p.lbase[k];
    if (t.t_base[r + 1] - b != C) { *bad = 1; return; }
    const int32_t *cs = t.t_cstart + b + r;
    int a = 0;
    p.lev[(int64_t)k * p.LW] = 0;
    for (int L = 1; L < p.LW; ++L) {
        const int nx = a < C ? cs[a] : (int)C;
        if (nx < a || nx > C) { *bad = 1; return; }
        a = nx;
        p.lev[(int64_t)k * p.LW + L] = a;
    }
    if (a != C) *bad = 1;
}

// one thread per rank at level L of every slot of the pass (lvoff: [P + 1] offsets of the slots' ranges of the level)
__global__ __launch_bounds__(256) void gs_level_kernel(GsTree t, GsPass p, int32_t L, const int64_t *lvoff, int64_t items) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= items) return;
    const int k = find_slot(lvoff, p.P, j);
    const int r = p.slots[k];
    const int i = p.lev[(int64_t)k * p.LW + L] + (int)(j - lvoff[k]);
    const int64_t b = t.t_base[r];
    const int32_t *cs = t.t_cstart + b + r;
    const int c0 = cs[i], c1 = cs[i + 1];
    if (c1 - c0 > GS_LONG) {
        const int q = atomicAdd(p.long_cnt + L, 1);
        p.long_list[q] = make_int2(k, i);
        return;
    }
    const bool hf = father_in(t, r, i, L);
    const double sf = hf ? t.es[t.g_rev[t.t_edge[b + i]]] : -INFINITY;
    double m = sf;
    for (int c = c0; c < c1; ++c) m = fmax(m, t.es[t.t_edge[b + c]]);
    if (c0 == c1 && !hf) return;  // N(v) empty: the walk aborts here (gs_abort_kernel)
    double s = hf ? exp(sf - m) : 0.0;
    for (int c = c0; c < c1; ++c) s += exp(t.es[t.t_edge[b + c]] - m);
    const double lse = m + log(s);
    const int64_t lb = p.lbase[k];
    const double lr = i == 0 ? 0.0 : p.logR[lb + i];
    for (int c = c0; c < c1; ++c) p.logR[lb + c] = lr + (t.es[t.t_edge[b + c]] - lse);
    if (hf) p.dense[(int64_t)k * p.n_node + t.t_order[b + i]] = (float)(lr + (sf - lse));
}

// one workgroup per queued rank of level L (a list of more than GS_LONG children): thread x takes children x, x + 256, ...;
// partial maxima and sums meet in a fixed LDS tree
__global__ __launch_bounds__(256) void gs_long_kernel(GsTree t, GsPass p, int32_t L) {
    __shared__ double red[256], redm[256];
    const int tid = threadIdx.x;
    const int cnt = p.long_cnt[L];
    for (int q = blockIdx.x; q < cnt; q += gridDim.x) {
        const int2 e = p.long_list[q];
        const int k = e.x, i = e.y, r = p.slots[k];
        const int64_t b = t.t_base[r];
        const int32_t *cs = t.t_cstart + b + r;
        const int c0 = cs[i], c1 = cs[i + 1];
        const bool hf = father_in(t, r, i, L);
        const double sf = hf ? t.es[t.g_rev[t.t_edge[b + i]]] : -INFINITY;
        double m = tid == 0 ? sf : -INFINITY;
        for (int c = c0 + tid; c < c1; c += 256) m = fmax(m, t.es[t.t_edge[b + c]]);
        redm[tid] = m;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) redm[tid] = fmax(redm[tid], redm[tid + w]);
            __syncthreads();
        }
        m = redm[0];
        double s = (tid == 0 && hf) ? exp(sf - m) : 0.0;
        for (int c = c0 + tid; c < c1; c += 256) s += exp(t.es[t.t_edge[b + c]] - m);
        red[tid] = s;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) red[tid] += red[tid + w];
            __syncthreads();
        }
        const double lse = m + log(red[0]);
        const int64_t lb = p.lbase[k];
        const double lr = i == 0 ? 0.0 : p.logR[lb + i];
        for (int c = c0 + tid; c < c1; c += 256) p.logR[lb + c] = lr + (t.es[t.t_edge[b + c]] - lse);
        if (tid == 0 && hf) p.dense[(int64_t)k * p.n_node + t.t_order[b + i]] = (float)(lr + (sf - lse));
        __syncthreads();  // (red / redm are reused by the next entry)
    }
}

// one wavefront per slot: the abort mass A.  N(v) can only be empty at the root (no children) or at a depth-1 leaf whose father
// entry is dropped, so A is a sum over level 1: lane x takes ranks 1 + x, 1 + x + 64, ..., then a fixed xor butterfly.
__global__ __launch_bounds__(64) void gs_abort_kernel(GsTree t, GsPass p, float *abort_out) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const int r = p.slots[k];
    const int64_t b = t.t_base[r], lb = p.lbase[k];
    const int64_t C = p.lbase[k + 1] - lb;
    const int32_t *cs = t.t_cstart + b + r;
    double s = 0.0;
    if (C == 1) {
        s = lane == 0 ? 1.0 : 0.0;
    } else {
        const int e1 = cs[1];
        for (int i = 1 + lane; i < e1; i += 64)
            if (cs[i + 1] == cs[i] && !father_in(t, r, i, 1)) s += exp(p.logR[lb + i]);
    }
    for (int w = 32; w > 0; w >>= 1) s += __shfl_xor(s, w, 64);
    if (lane == 0) abort_out[k] = (float)s;
}

// queried pairs of the pass: q_logp[j] = dense[k][q_node[j]] for qoff[k] <= j < qoff[k + 1]
__global__ __launch_bounds__(256) void gs_gather_kernel(const float *dense, int32_t n_node, const int64_t *qoff, int32_t P, const int32_t *qnode,
                                                        int64_t nq, float *out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nq) return;
    const int k = find_slot(qoff, P, j);
    out[j] = dense[(int64_t)k * n_node + qnode[j]];
}

}  // namespace

// The private edge scores of the generator's current tables (and the per-node chunk offsets of their fill, once per graph).
static int ensure_gs_scores(gg_ctx *ctx) {
    const int n = ctx->n_node;
    if (!ctx->gs_cpre_valid) {
        std::vector<int64_t> cpre((size_t)n + 1, 0);
        for (int v = 0; v < n; ++v) cpre[v + 1] = cpre[v] + (ctx->h_rowptr[v + 1] - ctx->h_rowptr[v] + 15) / 16;
        GG_HIP(ctx, ctx->gs_cpre.reserve(sizeof(int64_t) * (n + 1)));
        GG_HIP(ctx, hipMemcpy(ctx->gs_cpre.p, cpre.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice));
        ctx->gs_chunks = cpre[n];
        ctx->gs_cpre_valid = true;
    }
    if (ctx->gs_es_valid) return GG_OK;
    GG_HIP(ctx, ctx->gs_es.reserve(sizeof(double) * (size_t)std::max<int64_t>(ctx->g_nnz, 1)));
    if (ctx->gs_chunks > 0) {
        const Model &G = ctx->model[0];
        const int nchunk = ctx->ld / 4, nch = (nchunk + 15) / 16;
        const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((ctx->gs_chunks + 15) / 16, (int64_t)ctx->n_cus * 16));
        const int64_t *cp = ctx->gs_cpre.as<int64_t>();
        double *es = ctx->gs_es.as<double>();
#define GS_FILL(N) hipLaunchKernelGGL(gs_fill_kernel<N>, dim3(blocks), dim3(256), 0, ctx->stream, G.E, G.b, ctx->ld, nchunk, ctx->g_rowptr, ctx->g_col, cp, n, ctx->gs_chunks, es)
        if (nch <= 1) GS_FILL(1);
        else if (nch == 2) GS_FILL(2);
        else if (nch <= 4) GS_FILL(4);
        else GS_FILL(8);
#undef GS_FILL
        GG_HIP(ctx, hipGetLastError());
    }
    ctx->gs_es_valid = true;
    return GG_OK;
}

}  // namespace gg

using namespace gg;

// gg_graph_softmax: see include/graphgan_hip.h.
extern "C" int gg_graph_softmax(gg_ctx *ctx, const int32_t *slots, int32_t n_slots, int32_t flags, float *logp, const int64_t *q_off,
                                const int32_t *q_node, float *q_logp, float *abort_mass, double *kernel_ms_out) {
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    GG_CHECK(ctx, (flags & ~(GG_GS_FOR_D | GG_GS_Q3_STORE)) == 0, GG_EINVAL, "gg_graph_softmax: unknown flags 0x%x", flags);
    GG_CHECK(ctx, n_slots >= 0 && (slots || n_slots == 0), GG_EINVAL, "gg_graph_softmax: bad slots");
    GG_CHECK(ctx, !q_off == !q_logp, GG_EINVAL, "gg_graph_softmax: q_off and q_logp go together");
    discard_begun_walk(ctx);  // (a begun gg_prepare_g launch reads the trees and the generator: waited for and dropped)
    GG_CHECK(ctx, ctx->n_tree_roots > 0 || n_slots == 0, GG_EINVAL, "gg_graph_softmax: no trees loaded (gg_build_trees / gg_set_trees)");
    GG_CHECK(ctx, !ctx->t_lazy, GG_EINVAL,
             "gg_graph_softmax: the resident trees are lazy (exact through a level only): build them whole -- gg_set_tree_mode(ctx, 0) with node_cap 0 -- first");
    GG_CHECK(ctx, n_slots == 0 || (ctx->t_edge_valid && ctx->t_edge), GG_EINVAL,
             "gg_graph_softmax: the resident trees carry no edge indices (edges_valid == 0: lists that are no subgraph of the resident graph)");
    GG_CHECK(ctx, n_slots == 0 || ctx->g_rev, GG_EINVAL, "gg_graph_softmax: the resident graph has no reverse-edge index (not symmetric, or its edge-score cache did not fit)");
    for (int k = 0; k < n_slots; ++k)
        GG_CHECK(ctx, slots[k] >= 0 && slots[k] < ctx->n_tree_roots, GG_EINVAL, "gg_graph_softmax: slot %d out of range [0, %d)", slots[k], ctx->n_tree_roots);
    const int n = ctx->n_node;
    if (q_off) {
        GG_CHECK(ctx, q_off[0] == 0, GG_EINVAL, "gg_graph_softmax: q_off[0] must be 0");
        for (int k = 0; k < n_slots; ++k) GG_CHECK(ctx, q_off[k + 1] >= q_off[k], GG_EINVAL, "gg_graph_softmax: q_off not monotone at %d", k);
        GG_CHECK(ctx, q_node || q_off[n_slots] == 0, GG_EINVAL, "gg_graph_softmax: q_node is NULL");
        for (int64_t j = 0; j < q_off[n_slots]; ++j)
            GG_CHECK(ctx, q_node[j] >= 0 && q_node[j] < n, GG_EINVAL, "gg_graph_softmax: q_node[%lld] = %d out of range [0, %d)", (long long)j, q_node[j], n);
    }
    if (n_slots == 0) return GG_OK;
    GG_HIP(ctx, hipSetDevice(ctx->device));
    unsigned long long bad_table = 0;
    GG_HIP(ctx, hipMemcpyAsync(&bad_table, ctx->table_bad.p, sizeof(bad_table), hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    GG_CHECK(ctx, !bad_table, GG_EINVAL, "gg_graph_softmax: the generator's tables hold a non-finite value");
    int rc = ensure_gs_scores(ctx);
    if (rc != GG_OK) return rc;

    const int LW = ctx->tree_max_depth + 3;  // level starts 0 .. depth + 2 (the last two: the end of the tree)
    const int P_max = (int)std::max<int64_t>(1, std::min<int64_t>(GS_MAX_SLOTS, (int64_t)(GS_DENSE_BYTES / (sizeof(float) * (size_t)n))));
    const int chunk = std::min(P_max, n_slots);
    int64_t max_nodes = 0;  // most logR entries of one pass
    for (int k0 = 0; k0 < n_slots; k0 += chunk) {
        int64_t s = 0;
        for (int k = k0; k < std::min(n_slots, k0 + chunk); ++k) s += ctx->h_tbase[slots[k] + 1] - ctx->h_tbase[slots[k]];
        max_nodes = std::max(max_nodes, s);
    }
    int64_t max_q = 0;
    if (q_off)
        for (int k0 = 0; k0 < n_slots; k0 += chunk) max_q = std::max(max_q, q_off[std::min(n_slots, k0 + chunk)] - q_off[k0]);
    const bool stage_q3_store = (flags & GG_GS_Q3_STORE) != 0;
    GsTree t{ctx->t_root, ctx->t_order, ctx->t_cstart, ctx->t_edge, ctx->t_base, nullptr, nullptr, 0, ctx->g_rev, ctx->gs_es.as<double>(),
             (flags & GG_GS_FOR_D) ? 1 : 0};
    if (stage_q3_store) {
        if (ctx->q3_store_ready) { t.q3 = ctx->q3_store.as<uint32_t>(); t.q3off = ctx->q3s_off.as<int64_t>(); t.q3_by_node = 1; }
    } else {
        t.q3 = ctx->t_q3;
        t.q3off = ctx->t_q3off;
    }

    DevBuf d_slots, d_lbase, d_logR, d_lev, d_dense, d_lvoff, d_long, d_cnt, d_abort, d_qoff, d_qnode, d_q, d_bad;
    auto rel = [&]() {
        for (DevBuf *x : {&d_slots, &d_lbase, &d_logR, &d_lev, &d_dense, &d_lvoff, &d_long, &d_cnt, &d_abort, &d_qoff, &d_qnode, &d_q, &d_bad}) x->release();
    };
    hipError_t e = d_slots.reserve(sizeof(int32_t) * chunk);
    if (e == hipSuccess) e = d_lbase.reserve(sizeof(int64_t) * (chunk + 1));
    if (e == hipSuccess) e = d_logR.reserve(sizeof(double) * (size_t)std::max<int64_t>(max_nodes, 1));
    if (e == hipSuccess) e = d_lev.reserve(sizeof(int32_t) * (size_t)chunk * LW);
    if (e == hipSuccess) e = d_dense.reserve(sizeof(float) * (size_t)chunk * n);
    if (e == hipSuccess) e = d_lvoff.reserve(sizeof(int64_t) * (size_t)LW * (chunk + 1));
    if (e == hipSuccess) e = d_long.reserve(sizeof(int2) * (size_t)std::max<int64_t>(max_nodes, 1));
    if (e == hipSuccess) e = d_cnt.reserve(sizeof(int32_t) * LW);
    if (e == hipSuccess) e = d_abort.reserve(sizeof(float) * chunk);
    if (e == hipSuccess) e = d_bad.reserve(sizeof(int32_t));
    if (e == hipSuccess && q_off) e = d_qoff.reserve(sizeof(int64_t) * (chunk + 1));
    if (e == hipSuccess && q_off) e = d_qnode.reserve(sizeof(int32_t) * (size_t)std::max<int64_t>(max_q, 1));
    if (e == hipSuccess && q_off) e = d_q.reserve(sizeof(float) * (size_t)std::max<int64_t>(max_q, 1));
    if (e != hipSuccess) { rel(); return fail(ctx, GG_ENOMEM, "gg_graph_softmax: scratch: %s", hipGetErrorString(e)); }

    std::vector<int64_t> h_lbase, h_lvoff, h_qoff;
    std::vector<int32_t> h_lev;
    double ms_total = 0.0;
    for (int k0 = 0; k0 < n_slots && e == hipSuccess; k0 += chunk) {
        const int P = std::min(chunk, n_slots - k0);
        h_lbase.assign(P + 1, 0);
        for (int k = 0; k < P; ++k) h_lbase[k + 1] = h_lbase[k] + ctx->h_tbase[slots[k0 + k] + 1] - ctx->h_tbase[slots[k0 + k]];
        GsPass p{d_slots.as<int32_t>(), P, d_lbase.as<int64_t>(), d_logR.as<double>(), d_lev.as<int32_t>(), LW, d_dense.as<float>(), n,
                 d_long.as<int2>(), d_cnt.as<int32_t>()};
        int32_t h_bad = 0;
        e = hipMemcpyAsync(d_slots.p, slots + k0, sizeof(int32_t) * P, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_lbase.p, h_lbase.data(), sizeof(int64_t) * (P + 1), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_bad.p, 0, sizeof(int32_t), ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_cnt.p, 0, sizeof(int32_t) * LW, ctx->stream);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(gs_plan_kernel, dim3((unsigned)cdiv(P, 64)), dim3(64), 0, ctx->stream, t, p, d_bad.as<int32_t>());
        h_lev.resize((size_t)P * LW);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h_lev.data(), d_lev.p, sizeof(int32_t) * (size_t)P * LW, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&h_bad, d_bad.p, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) break;
        if (h_bad) { rel(); return fail(ctx, GG_EINVAL, "gg_graph_softmax: a resident tree does not match its recorded size / depth"); }
        // per level: the slots' rank ranges, prefix-summed (the launch of level L covers lvoff[L][P] ranks)
        h_lvoff.assign((size_t)LW * (P + 1), 0);
        for (int L = 0; L + 1 < LW; ++L)
            for (int k = 0; k < P; ++k)
                h_lvoff[(size_t)L * (P + 1) + k + 1] = h_lvoff[(size_t)L * (P + 1) + k] + (h_lev[(size_t)k * LW + L + 1] - h_lev[(size_t)k * LW + L]);
        e = hipMemcpyAsync(d_lvoff.p, h_lvoff.data(), sizeof(int64_t) * h_lvoff.size(), hipMemcpyHostToDevice, ctx->stream);
        int64_t nq = 0;
        if (e == hipSuccess && q_off) {
            nq = q_off[k0 + P] - q_off[k0];
            h_qoff.resize(P + 1);
            for (int k = 0; k <= P; ++k) h_qoff[k] = q_off[k0 + k] - q_off[k0];
            e = hipMemcpyAsync(d_qoff.p, h_qoff.data(), sizeof(int64_t) * (P + 1), hipMemcpyHostToDevice, ctx->stream);
            if (e == hipSuccess && nq) e = hipMemcpyAsync(d_qnode.p, q_node + q_off[k0], sizeof(int32_t) * nq, hipMemcpyHostToDevice, ctx->stream);
        }
        if (e != hipSuccess) break;
        (void)hipEventRecord(ctx->ev0, ctx->stream);
        const int64_t dn = (int64_t)P * n;
        hipLaunchKernelGGL(gs_fill_dense_kernel, dim3((unsigned)std::min<int64_t>(cdiv(dn, 256), (int64_t)ctx->n_cus * 16)), dim3(256), 0, ctx->stream,
                           d_dense.as<float>(), dn);
        for (int L = 0; L + 1 < LW; ++L) {
            const int64_t *lvo = d_lvoff.as<int64_t>() + (size_t)L * (P + 1);
            const int64_t items = h_lvoff[(size_t)L * (P + 1) + P];
            if (items == 0) continue;
            hipLaunchKernelGGL(gs_level_kernel, dim3((unsigned)cdiv(items, 256)), dim3(256), 0, ctx->stream, t, p, L, lvo, items);
            const int64_t long_blocks = std::min<int64_t>(cdiv(items, GS_LONG + 1), (int64_t)ctx->n_cus * 4);
            hipLaunchKernelGGL(gs_long_kernel, dim3((unsigned)std::max<int64_t>(long_blocks, 1)), dim3(256), 0, ctx->stream, t, p, L);
        }
        hipLaunchKernelGGL(gs_abort_kernel, dim3((unsigned)P), dim3(64), 0, ctx->stream, t, p, d_abort.as<float>());
        if (nq) hipLaunchKernelGGL(gs_gather_kernel, dim3((unsigned)cdiv(nq, 256)), dim3(256), 0, ctx->stream, d_dense.as<float>(), n, d_qoff.as<int64_t>(), P,
                                   d_qnode.as<int32_t>(), nq, d_q.as<float>());
        (void)hipEventRecord(ctx->ev1, ctx->stream);
        e = hipGetLastError();
        if (e == hipSuccess && logp) e = hipMemcpyAsync(logp + (int64_t)k0 * n, d_dense.p, sizeof(float) * (size_t)dn, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && nq) e = hipMemcpyAsync(q_logp + q_off[k0], d_q.p, sizeof(float) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && abort_mass) e = hipMemcpyAsync(abort_mass + k0, d_abort.p, sizeof(float) * P, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        float ms = 0.f;
        if (e == hipSuccess) (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
        ms_total += ms;
    }
    rel();
    if (e != hipSuccess) return fail(ctx, GG_EHIP, "gg_graph_softmax: %s", hipGetErrorString(e));
    if (kernel_ms_out) *kernel_ms_out = ms_total;
    return GG_OK;
}
