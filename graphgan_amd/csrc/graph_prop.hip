// graph_prop.hip -- the neighbour-sum sweep: every node sums the fp32 rows of its neighbours in the resident training graph,
//   H[v, c] = sum over w in N(v) of (in_scale[w] * X[w, c]),
// a CSR times dense-matrix product and the building block of propagation on the graph.  gg_neighbor_sum exposes it as a
// primitive; gg_label_spread iterates it with the label-spreading epilogue F' = a[v] * H + b * Y0 (Zhou et al. 2004).  No
// embedding table is read: a bandwidth-bound row gather over the SET adjacency of ensure_set_adjacency (pair_neighbors.hip).
//
// Shape (the first build; what was not tuned is listed in DESIGN.md "Neighbour-sum sweep"):
//   rows        padded on the device to CP = 4 ceil(n_col / 4) floats, so a row is CP / 4 16-byte loads;
//   LPR         lanes per row: the smallest power of two >= CP / 4 (instances 1 .. 32); lanes q >= CP / 4 of a group are padding:
//               they load nothing, carry exact zeros and store nothing;
//   a task      (request row i, first entry c0, stage row or -1) = the entries [c0, min(deg, c0 + GP_CHUNK)) of node v's list;
//   a wavefront takes a task: its G = 64 / LPR lane groups each take a different neighbour (e = c0 + g, c0 + g + G, ...), GP_ROUNDS
//               rows in flight per group before the first add, the ids of the next batch loaded ahead of the rows;
//   the fold    the groups' float4 accumulators are added by a fixed xor-shuffle tree (offsets LPR, 2 LPR, ..., 32);
//   a hub       deg > GP_CHUNK: ceil(deg / GP_CHUNK) tasks write partial rows into a stage, gp_hub_kernel adds them in ascending
//               chunk order and applies the epilogue.  Every other node has one task, which applies the epilogue itself.
// A node's adds therefore depend on its list, the gathered values and n_col alone -- not on the request, the grid or the run --
// and there is no floating-point atomic: the bits of a node's row are the same in every call.  The epilogue is a compile-time
// variant (EPI) of the ONE sweep kernel, so a fit of T iterations equals T primitive calls composed on the host, bit for bit.
#include <algorithm>

#include "set_sweep.h"

namespace gg {

namespace {

constexpr int GP_CHUNK = 512;     // entries of a node's list per task (Engine.NEIGHBOR_SUM_CHUNK)
constexpr int GP_ROUNDS = 4;      // rows in flight per lane group before the first add
constexpr int GP_BLOCKS = 2048;   // workgroups per launch at most (8 per CU); the wavefronts stride over the tasks behind them
constexpr int GP_MAX_COL = 128;

enum { EPI_SCALE = 0, EPI_SPREAD = 1 };

struct GpEpi {
    float *out;               // [m, CP]
    int n_col, CP;
    const float *out_scale;   // EPI_SCALE: [n_node] or NULL (no multiply)
    const float *a;           // EPI_SPREAD: [n_node]
    const uint32_t *bits;     //   [n_node, CW] label masks of every node (zero rows for the unlabelled)
    int CW;
    float b;
    const float *prev;        //   [n_node, CP] F_t, read for delta only
    unsigned int *delta;      //   max |F' - F_t| as the bits of a non-negative float, or NULL
};

struct GpArgs {
    const int4 *task;         // (i, c0, stage row or -1, 0)
    int n_task;
    const int32_t *nodes;     // [m] request row -> node, or NULL (the row is the node)
    const int64_t *ptr;       // set adjacency
    const int32_t *adj;
    const float *X;           // [n_node, CP]
    const float *in_scale;    // [n_node] or NULL (no multiply)
    float *stage;             // [stage rows, CP]
    GpEpi e;
};

// the epilogue of columns [col, col + 4) of node v (request row i) on its neighbour sum h; returns the quad's share of delta
template <int EPI>
__device__ __forceinline__ float gp_finish_quad(const GpEpi &e, int i, int v, int col, float4 h) {
    float r[4] = {h.x, h.y, h.z, h.w};
    float d = 0.f;
    if (EPI == EPI_SCALE) {
        if (e.out_scale) {
            const float os = e.out_scale[v];
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = __fmul_rn(os, r[k]);
        }
    } else {
        const float av = e.a[v];
        const uint32_t word = e.bits[(size_t)v * e.CW + (col >> 5)] >> (col & 31);  // (col is a multiple of 4: one word holds the quad)
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = __fadd_rn(__fmul_rn(av, r[k]), ((word >> k) & 1u) ? e.b : 0.f);
        if (e.delta) {
            const float4 p = *reinterpret_cast<const float4 *>(e.prev + (size_t)v * e.CP + col);
            d = fmaxf(fmaxf(fabsf(__fsub_rn(r[0], p.x)), fabsf(__fsub_rn(r[1], p.y))), fmaxf(fabsf(__fsub_rn(r[2], p.z)), fabsf(__fsub_rn(r[3], p.w))));
        }
    }
    float *dst = e.out + (size_t)i * e.CP + col;
    if (col + 4 <= e.n_col) {
        *reinterpret_cast<float4 *>(dst) = make_float4(r[0], r[1], r[2], r[3]);
    } else {  // the ragged last quad: the padding columns are never stored
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (col + k < e.n_col) dst[k] = r[k];
    }
    return d;
}

// the wavefront's largest |F' - F_t| into the delta word: an integer maximum of non-negative float bits, so order-independent
__device__ __forceinline__ void gp_delta_max(unsigned int *delta, float d) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) d = fmaxf(d, __shfl_xor(d, off, 64));
    if ((threadIdx.x & 63) == 0 && d > 0.f) atomicMax(delta, __float_as_uint(d));
}

template <int LPR, int EPI>
__global__ __launch_bounds__(256) void gp_sweep_kernel(GpArgs o) {
    constexpr int G = 64 / LPR;
    const int lane = threadIdx.x & 63, g = lane / LPR, col = (lane % LPR) * 4;
    const bool live = col < o.e.CP;
    const bool scaled = o.in_scale != nullptr;
    const int waves = gridDim.x * 4;
    float dmax = 0.f;
    for (int t = blockIdx.x * 4 + (threadIdx.x >> 6); t < o.n_task; t += waves) {  // (one task per wavefront: uniform trip counts)
        const int4 tk = o.task[t];
        const int i = tk.x, c0 = tk.y;
        const int v = o.nodes ? o.nodes[i] : i;
        const int64_t b0 = o.ptr[v];
        const int end = min((int)(o.ptr[v + 1] - b0), c0 + GP_CHUNK);
        const int32_t *A = o.adj + b0;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        int id[GP_ROUNDS];
#pragma unroll
        for (int r = 0; r < GP_ROUNDS; ++r) {
            const int e = c0 + r * G + g;
            id[r] = e < end ? A[e] : -1;
        }
        for (int base = c0; base < end; base += G * GP_ROUNDS) {
            float4 x[GP_ROUNDS];
            float sc[GP_ROUNDS];
#pragma unroll
            for (int r = 0; r < GP_ROUNDS; ++r) {  // every load of the batch is issued before the first add
                x[r] = (id[r] >= 0 && live) ? *reinterpret_cast<const float4 *>(o.X + (size_t)id[r] * o.e.CP + col) : make_float4(0.f, 0.f, 0.f, 0.f);
                sc[r] = (scaled && id[r] >= 0) ? o.in_scale[id[r]] : 0.f;
            }
            int nid[GP_ROUNDS];
#pragma unroll
            for (int r = 0; r < GP_ROUNDS; ++r) {  // the ids of the next batch, ahead of its rows
                const int e = base + (GP_ROUNDS + r) * G + g;
                nid[r] = e < end ? A[e] : -1;
            }
#pragma unroll
            for (int r = 0; r < GP_ROUNDS; ++r) {
                if (scaled) x[r] = make_float4(__fmul_rn(sc[r], x[r].x), __fmul_rn(sc[r], x[r].y), __fmul_rn(sc[r], x[r].z), __fmul_rn(sc[r], x[r].w));
                acc = make_float4(__fadd_rn(acc.x, x[r].x), __fadd_rn(acc.y, x[r].y), __fadd_rn(acc.z, x[r].z), __fadd_rn(acc.w, x[r].w));
                id[r] = nid[r];
            }
        }
#pragma unroll
        for (int off = LPR; off < 64; off <<= 1)  // the fixed tree over the lane groups (a + b == b + a: every lane ends with the same bits)
            acc = make_float4(__fadd_rn(acc.x, __shfl_xor(acc.x, off, 64)), __fadd_rn(acc.y, __shfl_xor(acc.y, off, 64)),
                              __fadd_rn(acc.z, __shfl_xor(acc.z, off, 64)), __fadd_rn(acc.w, __shfl_xor(acc.w, off, 64)));
        if (g == 0 && live) {
            if (tk.z >= 0) *reinterpret_cast<float4 *>(o.stage + (size_t)tk.z * o.e.CP + col) = acc;  // a hub's chunk: the partial row
            else dmax = fmaxf(dmax, gp_finish_quad<EPI>(o.e, i, v, col, acc));
        }
    }
    if (EPI == EPI_SPREAD && o.e.delta) gp_delta_max(o.e.delta, dmax);
}

// hubs: hub[h] = (i, first stage row, chunks, 0); one thread per (hub, quad) adds the partial rows in ascending chunk order
template <int EPI>
__global__ __launch_bounds__(256) void gp_hub_kernel(const int4 *hub, int n_hub, const int32_t *nodes, const float *stage, GpEpi e) {
    const int quads = e.CP / 4;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float d = 0.f;
    if (tid < (int64_t)n_hub * quads) {
        const int4 hb = hub[tid / quads];
        const int col = (int)(tid % quads) * 4;
        float4 acc = *reinterpret_cast<const float4 *>(stage + (size_t)hb.y * e.CP + col);
        for (int k = 1; k < hb.z; ++k) {
            const float4 p = *reinterpret_cast<const float4 *>(stage + (size_t)(hb.y + k) * e.CP + col);
            acc = make_float4(__fadd_rn(acc.x, p.x), __fadd_rn(acc.y, p.y), __fadd_rn(acc.z, p.z), __fadd_rn(acc.w, p.w));
        }
        d = gp_finish_quad<EPI>(e, hb.x, nodes ? nodes[hb.x] : hb.x, col, acc);
    }
    if (EPI == EPI_SPREAD && e.delta) gp_delta_max(e.delta, d);
}

// Y0 and the all-node label masks from the training nodes' masks: F[node, c] = 1 for every set bit (F and bits were zeroed)
__global__ __launch_bounds__(256) void gp_y0_kernel(const int32_t *train, const uint32_t *tbits, int64_t m, int CW, int CP, uint32_t *bits, float *F) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (tid >= m * CW) return;
    const int node = train[tid / CW], w = (int)(tid % CW);
    uint32_t word = tbits[tid];
    bits[(size_t)node * CW + w] = word;
    while (word) {
        const int c = __ffs(word) - 1;
        word &= word - 1;
        F[(size_t)node * CP + 32 * w + c] = 1.f;
    }
}

// out[i, :] = F[nodes[i], :] (padded rows, float4 per thread)
__global__ __launch_bounds__(256) void gp_rows_kernel(const float *F, const int32_t *nodes, int64_t m, int CP, float *out) {
    const int quads = CP / 4;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (tid >= m * quads) return;
    const int64_t i = tid / quads;
    const int col = (int)(tid % quads) * 4;
    *reinterpret_cast<float4 *>(out + (size_t)i * CP + col) = *reinterpret_cast<const float4 *>(F + (size_t)nodes[i] * CP + col);
}

// The tasks of a request: the chunk tasks of the hubs first (the longest work starts first), then one task per other node.
// (Not set_sweep.h's planner: one width, hubs ahead of the rest, and every chunk task carries its stage row.)
struct Plan {
    std::vector<int4> task, hub;
    int64_t n_stage = 0;
};

bool build_plan(const int64_t *hp, const int32_t *nodes, int64_t m, Plan &p) {
    std::vector<int4> direct;
    direct.reserve((size_t)m);
    for (int64_t i = 0; i < m; ++i) {
        const int v = nodes ? nodes[i] : (int)i;
        const int64_t len = hp[v + 1] - hp[v];
        if (len <= GP_CHUNK) {
            direct.push_back(make_int4((int)i, 0, -1, 0));
            continue;
        }
        const int chunks = cdiv(len, GP_CHUNK);
        if (p.n_stage + chunks > 0x7fffffffLL) return false;
        p.hub.push_back(make_int4((int)i, (int)p.n_stage, chunks, 0));
        for (int k = 0; k < chunks; ++k) p.task.push_back(make_int4((int)i, k * GP_CHUNK, (int)p.n_stage + k, 0));
        p.n_stage += chunks;
    }
    if (p.task.size() + direct.size() > 0x7fffffffull) return false;
    p.task.insert(p.task.end(), direct.begin(), direct.end());
    return true;
}

int upload_plan(gg_ctx *ctx, const char *fn, const Plan &p, DevBuf &d_task, DevBuf &d_hub, DevSumPlan &dp) {
    hipError_t e = d_task.reserve(sizeof(int4) * std::max<size_t>(p.task.size(), 1));
    if (e == hipSuccess) e = d_hub.reserve(sizeof(int4) * std::max<size_t>(p.hub.size(), 1));
    if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "%s: %s", fn, hipGetErrorString(e));
    if (!p.task.empty()) GG_HIP_FN(hipMemcpyAsync(d_task.p, p.task.data(), sizeof(int4) * p.task.size(), hipMemcpyHostToDevice, ctx->stream));
    if (!p.hub.empty()) GG_HIP_FN(hipMemcpyAsync(d_hub.p, p.hub.data(), sizeof(int4) * p.hub.size(), hipMemcpyHostToDevice, ctx->stream));
    GG_HIP_FN(hipStreamSynchronize(ctx->stream));  // (the host vectors end with the caller's scope)
    dp.task = d_task.as<int4>();
    dp.hub = d_hub.as<int4>();
    dp.n_task = (int)p.task.size();
    dp.n_hub = (int)p.hub.size();
    dp.n_stage = p.n_stage;
    return GG_OK;
}

// The plan of the all-nodes sweep is a function of the graph: built once behind the set adjacency, kept in the context and
// dropped by gg_set_graph_csr (SetGraph::drop): ctx->set.sum.
int ensure_sweep_plan(gg_ctx *ctx, const char *fn) {
    const int rc = ensure_set_adjacency(ctx);
    if (rc != GG_OK) return rc;
    SetGraph &g = ctx->set;
    if (g.sum_valid) return GG_OK;
    Plan p;
    GG_CHECK(ctx, build_plan(g.h_ptr.data(), nullptr, ctx->n_node, p), GG_EINVAL, "%s: too many tasks", fn);
    const int rc2 = upload_plan(ctx, fn, p, g.gp_task, g.gp_hub, g.sum);
    if (rc2 != GG_OK) return rc2;
    g.sum_valid = true;
    return GG_OK;
}

template <int EPI>
void launch_sweep(hipStream_t stream, int lpr, const GpArgs &o, const DevSumPlan &dp) {
    if (o.n_task) {
        const dim3 grid(std::min(GP_BLOCKS, cdiv(o.n_task, 4))), block(256);
        switch (lpr) {
        case 1: hipLaunchKernelGGL((gp_sweep_kernel<1, EPI>), grid, block, 0, stream, o); break;
        case 2: hipLaunchKernelGGL((gp_sweep_kernel<2, EPI>), grid, block, 0, stream, o); break;
        case 4: hipLaunchKernelGGL((gp_sweep_kernel<4, EPI>), grid, block, 0, stream, o); break;
        case 8: hipLaunchKernelGGL((gp_sweep_kernel<8, EPI>), grid, block, 0, stream, o); break;
        case 16: hipLaunchKernelGGL((gp_sweep_kernel<16, EPI>), grid, block, 0, stream, o); break;
        default: hipLaunchKernelGGL((gp_sweep_kernel<32, EPI>), grid, block, 0, stream, o); break;
        }
    }
    if (dp.n_hub)
        hipLaunchKernelGGL((gp_hub_kernel<EPI>), dim3(cdiv((int64_t)dp.n_hub * (o.e.CP / 4), 256)), dim3(256), 0, stream, dp.hub, dp.n_hub, o.nodes, o.stage, o.e);
}

int lanes_per_row(int CP) {
    int lpr = 1;
    while (lpr < CP / 4) lpr <<= 1;
    return lpr;
}

// host rows [rows, n_col] <-> device rows [rows, CP], on the stream
hipError_t copy_rows(void *dst, size_t dpitch, const void *src, size_t spitch, int n_col, int64_t rows, hipMemcpyKind kind, hipStream_t stream) {
    if (rows == 0) return hipSuccess;
    if (dpitch == spitch) return hipMemcpyAsync(dst, src, dpitch * (size_t)rows, kind, stream);
    return hipMemcpy2DAsync(dst, dpitch, src, spitch, sizeof(float) * (size_t)n_col, (size_t)rows, kind, stream);
}

}  // namespace

}  // namespace gg

using namespace gg;

// gg_neighbor_sum, gg_label_spread: see include/graphgan_hip.h.
extern "C" int gg_neighbor_sum(gg_ctx *ctx, const float *X, int32_t n_col, const float *in_scale, const float *out_scale, const int32_t *nodes, int64_t m,
                               float *out, double *kernel_ms) {
    const char *fn = "gg_neighbor_sum";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (kernel_ms) *kernel_ms = 0.0;
    GG_CHECK(ctx, ctx->g_rowptr, GG_EINVAL, "%s: needs the training graph (gg_set_graph_csr)", fn);
    GG_CHECK(ctx, n_col >= 1 && n_col <= GP_MAX_COL, GG_EINVAL, "%s: n_col = %d outside [1, %d]", fn, n_col, GP_MAX_COL);
    const int n = ctx->n_node;
    if (!nodes) m = n;
    GG_CHECK(ctx, m >= 0, GG_EINVAL, "%s: m = %lld is negative", fn, (long long)m);
    if (m == 0) return GG_OK;
    GG_CHECK(ctx, X && out, GG_EINVAL, "%s: X and out must not be NULL", fn);
    GG_CHECK(ctx, m <= 0x7fffffffLL, GG_EINVAL, "%s: m = %lld does not fit in 31 bits", fn, (long long)m);
    if (nodes) {
        const int rc = check_ids(ctx, fn, "nodes", nodes, m);
        if (rc != GG_OK) return rc;
    }
    GG_HIP(ctx, hipSetDevice(ctx->device));
    DevSumPlan own;  // the plan of a request of some nodes
    ScopedBuf d_task, d_hub;
    if (nodes) {
        const int rc = ensure_set_adjacency(ctx);
        if (rc != GG_OK) return rc;
        Plan p;
        GG_CHECK(ctx, build_plan(ctx->set.h_ptr.data(), nodes, m, p), GG_EINVAL, "%s: too many tasks", fn);
        const int rc2 = upload_plan(ctx, fn, p, d_task, d_hub, own);
        if (rc2 != GG_OK) return rc2;
    } else {
        const int rc = ensure_sweep_plan(ctx, fn);
        if (rc != GG_OK) return rc;
    }
    const DevSumPlan &dp = nodes ? own : ctx->set.sum;
    const int CP = 4 * cdiv(n_col, 4);
    const size_t row = sizeof(float) * CP;
    ScopedBuf d_X, d_out, d_in, d_os, d_nodes;
    hipError_t e = d_X.reserve(row * n);
    if (e == hipSuccess) e = d_out.reserve(row * (size_t)m);
    if (e == hipSuccess && in_scale) e = d_in.reserve(sizeof(float) * n);
    if (e == hipSuccess && out_scale) e = d_os.reserve(sizeof(float) * n);
    if (e == hipSuccess && nodes) e = d_nodes.reserve(sizeof(int32_t) * (size_t)m);
    if (e == hipSuccess) e = ctx->set.gp_stage.reserve(row * std::max<int64_t>(dp.n_stage, 1));
    if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "%s: %s", fn, hipGetErrorString(e));
    if (CP != n_col) GG_HIP_FN(hipMemsetAsync(d_X.p, 0, row * n, ctx->stream));  // (the padding columns are exact zeros)
    GG_HIP_FN(copy_rows(d_X.p, row, X, sizeof(float) * n_col, n_col, n, hipMemcpyHostToDevice, ctx->stream));
    if (in_scale) GG_HIP_FN(hipMemcpyAsync(d_in.p, in_scale, sizeof(float) * n, hipMemcpyHostToDevice, ctx->stream));
    if (out_scale) GG_HIP_FN(hipMemcpyAsync(d_os.p, out_scale, sizeof(float) * n, hipMemcpyHostToDevice, ctx->stream));
    if (nodes) GG_HIP_FN(hipMemcpyAsync(d_nodes.p, nodes, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    GpArgs o{};
    o.task = dp.task;
    o.n_task = dp.n_task;
    o.nodes = nodes ? d_nodes.as<int32_t>() : nullptr;
    o.ptr = ctx->set.ptr.as<int64_t>();
    o.adj = ctx->set.adj.as<int32_t>();
    o.X = d_X.as<float>();
    o.in_scale = in_scale ? d_in.as<float>() : nullptr;
    o.stage = ctx->set.gp_stage.as<float>();
    o.e.out = d_out.as<float>();
    o.e.n_col = n_col;
    o.e.CP = CP;
    o.e.out_scale = out_scale ? d_os.as<float>() : nullptr;
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    launch_sweep<EPI_SCALE>(ctx->stream, lanes_per_row(CP), o, dp);
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    GG_HIP_FN(hipGetLastError());
    GG_HIP_FN(copy_rows(out, sizeof(float) * n_col, d_out.p, row, n_col, m, hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    if (kernel_ms) *kernel_ms = ms;
    return GG_OK;
}

extern "C" int gg_label_spread(gg_ctx *ctx, const int32_t *train_nodes, const uint32_t *label_bits, int64_t m_train, int32_t n_class, double alpha,
                               int32_t iters, const float *s, const float *a, const int32_t *out_nodes, int64_t m_out, float *F_out, float *delta,
                               double *kernel_ms) {
    const char *fn = "gg_label_spread";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (kernel_ms) *kernel_ms = 0.0;
    GG_CHECK(ctx, ctx->g_rowptr, GG_EINVAL, "%s: needs the training graph (gg_set_graph_csr)", fn);
    GG_CHECK(ctx, n_class >= 1 && n_class <= GP_MAX_COL, GG_EINVAL, "%s: n_class = %d outside [1, %d]", fn, n_class, GP_MAX_COL);
    GG_CHECK(ctx, m_train >= 0, GG_EINVAL, "%s: m_train = %lld is negative", fn, (long long)m_train);
    const int n = ctx->n_node;
    if (!out_nodes) m_out = n;
    GG_CHECK(ctx, m_out >= 0, GG_EINVAL, "%s: m_out = %lld is negative", fn, (long long)m_out);
    GG_CHECK(ctx, m_out <= 0x7fffffffLL, GG_EINVAL, "%s: m_out = %lld does not fit in 31 bits", fn, (long long)m_out);
    GG_CHECK(ctx, train_nodes && label_bits, GG_EINVAL, "%s: train_nodes and label_bits must not be NULL", fn);
    GG_CHECK(ctx, s && a, GG_EINVAL, "%s: s and a must not be NULL", fn);
    GG_CHECK(ctx, m_out == 0 || F_out, GG_EINVAL, "%s: F_out must not be NULL", fn);
    GG_CHECK(ctx, alpha > 0.0 && alpha < 1.0, GG_EINVAL, "%s: alpha = %g outside (0, 1)", fn, alpha);
    GG_CHECK(ctx, iters >= 1, GG_EINVAL, "%s: iters = %d is below 1", fn, iters);
    int rc = check_ids(ctx, fn, "train_nodes", train_nodes, m_train);
    if (rc != GG_OK) return rc;
    {
        std::vector<int64_t> seen((size_t)n, -1);
        for (int64_t j = 0; j < m_train; ++j) {
            int64_t &first = seen[(size_t)train_nodes[j]];
            GG_CHECK(ctx, first < 0, GG_EINVAL, "%s: train_nodes[%lld] = %d repeats train_nodes[%lld]", fn, (long long)j, train_nodes[j], (long long)first);
            first = j;
        }
    }
    const int CW = cdiv(n_class, 32);
    if (n_class % 32)
        for (int64_t j = 0; j < m_train; ++j)
            GG_CHECK(ctx, (label_bits[j * CW + CW - 1] >> (n_class % 32)) == 0, GG_EINVAL, "%s: label_bits row %lld has a bit set at a position >= n_class = %d", fn,
                     (long long)j, n_class);
    if (out_nodes) {
        rc = check_ids(ctx, fn, "out_nodes", out_nodes, m_out);
        if (rc != GG_OK) return rc;
    }
    GG_HIP(ctx, hipSetDevice(ctx->device));
    rc = ensure_sweep_plan(ctx, fn);
    if (rc != GG_OK) return rc;
    const DevSumPlan &dp = ctx->set.sum;
    const int CP = 4 * cdiv(n_class, 4);
    const size_t row = sizeof(float) * CP;
    // the state lives on the device for the whole call: F_t and F_{t+1} (ping-pong), the label masks of every node (Y0 as bits)
    ScopedBuf d_F[2], d_bits, d_s, d_a, d_train, d_tbits, d_delta, d_onodes, d_orows;
    hipError_t e = d_F[0].reserve(row * n);
    if (e == hipSuccess) e = d_F[1].reserve(row * n);
    if (e == hipSuccess) e = d_bits.reserve(sizeof(uint32_t) * (size_t)CW * n);
    if (e == hipSuccess) e = d_s.reserve(sizeof(float) * n);
    if (e == hipSuccess) e = d_a.reserve(sizeof(float) * n);
    if (e == hipSuccess) e = d_train.reserve(sizeof(int32_t) * std::max<int64_t>(m_train, 1));
    if (e == hipSuccess) e = d_tbits.reserve(sizeof(uint32_t) * (size_t)CW * std::max<int64_t>(m_train, 1));
    if (e == hipSuccess) e = d_delta.reserve(sizeof(unsigned int));
    if (e == hipSuccess && out_nodes && m_out) e = d_onodes.reserve(sizeof(int32_t) * (size_t)m_out);
    if (e == hipSuccess && out_nodes && m_out) e = d_orows.reserve(row * (size_t)m_out);
    if (e == hipSuccess) e = ctx->set.gp_stage.reserve(row * std::max<int64_t>(dp.n_stage, 1));
    if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "%s: %s", fn, hipGetErrorString(e));
    GG_HIP_FN(hipMemcpyAsync(d_s.p, s, sizeof(float) * n, hipMemcpyHostToDevice, ctx->stream));
    GG_HIP_FN(hipMemcpyAsync(d_a.p, a, sizeof(float) * n, hipMemcpyHostToDevice, ctx->stream));
    if (m_train) {
        GG_HIP_FN(hipMemcpyAsync(d_train.p, train_nodes, sizeof(int32_t) * (size_t)m_train, hipMemcpyHostToDevice, ctx->stream));
        GG_HIP_FN(hipMemcpyAsync(d_tbits.p, label_bits, sizeof(uint32_t) * (size_t)CW * m_train, hipMemcpyHostToDevice, ctx->stream));
    }
    GG_HIP_FN(hipMemsetAsync(d_F[0].p, 0, row * n, ctx->stream));
    GG_HIP_FN(hipMemsetAsync(d_F[1].p, 0, row * n, ctx->stream));  // (its padding columns are read as part of a quad and never written)
    GG_HIP_FN(hipMemsetAsync(d_bits.p, 0, sizeof(uint32_t) * (size_t)CW * n, ctx->stream));
    GG_HIP_FN(hipMemsetAsync(d_delta.p, 0, sizeof(unsigned int), ctx->stream));
    if (m_train)
        hipLaunchKernelGGL(gp_y0_kernel, dim3(cdiv(m_train * CW, 256)), dim3(256), 0, ctx->stream, d_train.as<int32_t>(), d_tbits.as<uint32_t>(), m_train, CW, CP,
                           d_bits.as<uint32_t>(), d_F[0].as<float>());
    GpArgs o{};
    o.task = dp.task;
    o.n_task = dp.n_task;
    o.ptr = ctx->set.ptr.as<int64_t>();
    o.adj = ctx->set.adj.as<int32_t>();
    o.in_scale = d_s.as<float>();
    o.stage = ctx->set.gp_stage.as<float>();
    o.e.n_col = n_class;
    o.e.CP = CP;
    o.e.a = d_a.as<float>();
    o.e.bits = d_bits.as<uint32_t>();
    o.e.CW = CW;
    o.e.b = (float)(1.0 - alpha);
    const int lpr = lanes_per_row(CP);
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    for (int t = 0; t < iters; ++t) {  // the plan, the scales and the masks stay where they are: an iteration is its kernels
        o.X = d_F[t & 1].as<float>();
        o.e.out = d_F[(t + 1) & 1].as<float>();
        o.e.prev = o.X;
        o.e.delta = t == iters - 1 ? d_delta.as<unsigned int>() : nullptr;
        launch_sweep<EPI_SPREAD>(ctx->stream, lpr, o, dp);
    }
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    GG_HIP_FN(hipGetLastError());
    const float *F = d_F[iters & 1].as<float>();
    if (out_nodes && m_out) {
        GG_HIP_FN(hipMemcpyAsync(d_onodes.p, out_nodes, sizeof(int32_t) * (size_t)m_out, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(gp_rows_kernel, dim3(cdiv(m_out * (CP / 4), 256)), dim3(256), 0, ctx->stream, F, d_onodes.as<int32_t>(), m_out, CP, d_orows.as<float>());
        GG_HIP_FN(hipGetLastError());
        F = d_orows.as<float>();
    }
    GG_HIP_FN(copy_rows(F_out, sizeof(float) * n_class, F, row, n_class, m_out, hipMemcpyDeviceToHost, ctx->stream));
    if (delta) GG_HIP_FN(hipMemcpyAsync(delta, d_delta.p, sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    if (kernel_ms) *kernel_ms = ms;
    return GG_OK;
}
