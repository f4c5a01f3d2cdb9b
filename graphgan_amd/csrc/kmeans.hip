// kmeans.hip -- node clustering: Lloyd's k-means on rows of a resident table, gathered by node id.
//     a_i = argmin_c |x_i - c_c|^2 = argmin_c g_ic,   g_ic = h_c - x_i . c_c,   h_c = |c_c|^2 / 2     (ties: the lowest c)
//     dist2_i = max(0, |x_i|^2 + 2 g_{i, a_i}),   inertia = sum_i dist2_i
//     S_c = sum_{a_i = c} x_i,   n_c = |{i : a_i = c}|,   c_c <- S_c / n_c   (an empty cluster keeps its centroid)
// km_sweep_kernel is the hot path: the row-tile sweep of row_tiles.h (gather, D = Xs . Cs^T with the centroids as the staged
// operand, row stage, S += P^T . Xs; the geometry, the barriers and the launch plan are described there) with this file's row
// stage: per row, by 4 threads, |x_i|^2, the argmin of h_c - D_ic over c < k, dist2_i; the row's assignment and distance are
// written out, the inertia term goes to a float64 accumulator, `changed` counts a_i != the previous assignment; P = onehot(a_i)
// is left in LDS; n_c += column sums of P, as integers.
// The factors of the second product are 0 and 1: the matrix instruction is a k-ordered chain of fmaf, and fmaf(1, x, s) = s + x,
// fmaf(0, x, s) = s exactly, so S_c is the plain float32 sum of the cluster's rows in tile order -- no product is ever rounded.
// SUMS = false drops P, the counts and the second product (the assign-only calls: distances for seeding); the rest is the same
// code, the same bits.
// Every workgroup writes its partial (sums [k d] + the inertia as (high, remainder) floats; counts [k] + changed as integers) to
// a stage and km_update_kernel adds the stage in a fixed order.  No floating-point atomics: the same inputs give the same bits.
// km_update_kernel also applies the centroid update of a fit and owns its stop rule: ctl[0] = the sweep number the fit stopped
// at (0 while it runs), ctl[1] = converged.  A sweep or update of a later iteration finds ctl[0] set and returns at once, so all
// max_iters iterations are enqueued behind one another and the host synchronises once.
#include <math.h>

#include <algorithm>

#include "row_tiles.h"

namespace gg {

namespace {

constexpr int KM_RED_COLS = 32, KM_RED_SLICES = 8;  // km_update_kernel: entries x stage slices per workgroup

// has a fit stopped before iteration t?  (ctl[0] = the sweep it stopped at; the update kernel of sweep t itself may see t)
__device__ __forceinline__ bool km_stopped(const int32_t *ctl, int t) {
    const int32_t s = ctl[0];
    return s != 0 && s < t;
}

struct KmArgs {
    const float *E;          // [n_node, ld]
    const int32_t *nodes;
    int64_t m;
    int ld, d, k;
    const float *cen;        // [k, d]
    int KW;                  // k-chunk of the centroid staging (>= ld: staged once)
    float *part_f;           // [grid][k d + 2]: sums, the inertia as (high, remainder)
    int32_t *part_i;         // [grid][k + 1]: counts, changed
    int32_t *assign;         // [m] or NULL: in -- the previous assignment (has_prev), out -- this sweep's
    float *dist2;            // [m] or NULL
    int has_prev;
    const int32_t *ctl;      // the fit's stop words
    int t;                   // sweep number, from 1
};

template <int CT, int DT, bool SUMS>
__global__ __launch_bounds__(256) void km_sweep_kernel(KmArgs a) {
    constexpr int XS = RowTiles<CT, DT>::XS, PS = RowTiles<CT, DT>::PS;
    extern __shared__ float km_lds[];
    __shared__ float hs[RT_MAX_OUT];  // h_c = |c_c|^2 / 2
    __shared__ double red[256];     // the workgroup's inertia terms (float64: a sum of M terms must keep the last digits)
    __shared__ int redi[256];
    if (km_stopped(a.ctl, a.t)) return;
    const int tid = threadIdx.x, d = a.d, k = a.k;
    double inertia_acc = 0.0;
    int cnt_acc = 0, changed_acc = 0;

    // h_c: one thread per centroid, columns ascending (the order is part of the result; every workgroup computes the same bits).
    // From the staged copy where it is resident (odd row stride: conflict-free; the padding columns add +0), else from global
    // memory; either way the loads of 8 columns are issued together.
    auto half_norm = [&](const float *c, int n) {
        float s = 0.f;
        int j = 0;
        for (; j + 8 <= n; j += 8) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = c[j + e];
#pragma unroll
            for (int e = 0; e < 8; ++e) s += v[e] * v[e];
        }
        for (; j < n; ++j) s += c[j] * c[j];
        return 0.5f * s;
    };
    auto setup = [&](const float *Cs, int WS, bool resident) {
        if (resident) __syncthreads();
        if (tid < k) hs[tid] = resident ? half_norm(Cs + tid * WS, a.ld) : half_norm(a.cen + (int64_t)tid * d, d);  // (ld: a multiple of 4)
    };

    // row tid >> 2 by 4 threads (columns / clusters q, q + 4, ...): |x|^2, the argmin with ties to the lowest cluster
    auto rows = [&](int64_t row0, const float *Xs, float *Ps) {
        const int r = tid >> 2, q = tid & 3;
        const bool valid = row0 + r < a.m;
        float *p = Ps + r * PS;
        const float *x = Xs + r * XS;
        // |x|^2: thread q takes columns 32 b + 8 q + j (bank r + 8 q + j: the 32 lanes of a half hit 32 banks; columns behind
        // ld hold zeros), 8 loads issued together -- one wavefront per SIMD hides no LDS latency behind another
        float x2 = 0.f;
#pragma unroll
        for (int b = 0; b < DT; ++b) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = x[32 * b + 8 * q + j];
#pragma unroll
            for (int j = 0; j < 8; ++j) x2 += v[j] * v[j];
        }
        x2 += __shfl_xor(x2, 1);
        x2 += __shfl_xor(x2, 2);
        float best = INFINITY;
        int bc = 0x7fffffff;
#pragma unroll
        for (int b = 0; b < CT; ++b) {  // (the thread's clusters ascend: a later equal score does not replace)
            float g[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = 32 * b + q + 4 * j;  // (hs has RT_MAX_OUT entries and Ps 32 CT columns: every load is in bounds)
                const float hv = hs[c], pv = p[c];
                g[j] = c < k ? hv - pv : INFINITY;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (g[j] < best) {
                    best = g[j];
                    bc = 32 * b + q + 4 * j;
                }
        }
#pragma unroll
        for (int o = 1; o < 4; o <<= 1) {
            const float ob = __shfl_xor(best, o);
            const int oc = __shfl_xor(bc, o);
            if (ob < best || (ob == best && oc < bc)) {
                best = ob;
                bc = oc;
            }
        }
        if (bc >= k) bc = 0;  // no score compared below +inf (a row of NaN): cluster 0; nothing outside [0, k) leaves here
        const float dist2 = fmaxf(0.f, x2 + 2.f * best);
        if (q == 0 && valid) {
            inertia_acc += (double)dist2;
            if (a.has_prev) changed_acc += a.assign[row0 + r] != bc ? 1 : 0;
            if (a.assign) a.assign[row0 + r] = bc;
            if (a.dist2) a.dist2[row0 + r] = dist2;
        }
        // P = onehot(a_i): every thread rewrites the columns it has read
        if constexpr (SUMS)
            for (int c = q; c < 32 * CT; c += 4) p[c] = (valid && c == bc) ? 1.f : 0.f;
    };
    auto column = [&](float p) { cnt_acc += p != 0.f ? 1 : 0; };
    // the workgroup's partial
    float *part = a.part_f + (int64_t)blockIdx.x * ((int64_t)k * d + 2);
    int32_t *parti = a.part_i + (int64_t)blockIdx.x * (k + 1);
    row_tile_sweep<CT, DT, SUMS>(km_lds, a.E, a.nodes, a.m, a.ld, d, k, a.cen, a.KW, part, setup, rows, column);
    if constexpr (SUMS)
        if (tid < k) parti[tid] = cnt_acc;
    rt_block_sum(red, inertia_acc, part + (int64_t)k * d, redi, changed_acc, parti + k);
}

// The totals of a sweep from its stage, and -- in a fit (max_iters > 0) -- the centroid update and the stop rule.
//   sums[j], j < k d: a workgroup takes KM_RED_COLS entries, KM_RED_SLICES threads per entry sum contiguous slices of the stage
//     (and the integer counts of the entry's cluster), thread 0 of the entry adds the slices in order (nc_reduce_kernel's scheme);
//     with_sums = 0 (the assign-only sweep): these workgroups are not launched.
//   The LAST workgroup: counts[c] (integer sums), *inertia = the float64 sum of the (high, remainder) pairs by strided sums and a
//     fixed tree, and the fit's stop words.
// Every workgroup adds the integer `changed` words itself, so all take the same decision after sweep t:
//     t >= 2 and changed == 0 -> stop, converged;   else t == max_iters -> stop, not converged;   else apply the update
//     cen[c][j] = sums[c][j] / (float)counts[c] (one IEEE division), cen[c] untouched where counts[c] == 0.
__global__ __launch_bounds__(256) void km_update_kernel(const float *part_f, const int32_t *part_i, int n_part, int k, int d, int with_sums, float *cen,
                                                       float *sums, int32_t *counts, double *inertia, int32_t *ctl, int t, int max_iters) {
    __shared__ float sh[256];
    __shared__ int shi[256];
    __shared__ double shd[256];
    if (km_stopped(ctl, t)) return;
    const int tid = threadIdx.x;
    const int64_t kd = (int64_t)k * d, fs = kd + 2;
    const int is = k + 1;
    int ch = 0;
    for (int g = tid; g < n_part; g += 256) ch += part_i[(int64_t)g * is + k];
    shi[tid] = ch;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) shi[tid] += shi[tid + w];
        __syncthreads();
    }
    const int changed = shi[0];
    __syncthreads();
    const bool converged = t >= 2 && changed == 0;
    const bool stop = max_iters > 0 && (converged || t == max_iters);
    const bool apply = max_iters > 0 && !stop;
    if (blockIdx.x == gridDim.x - 1) {
        if (with_sums)
            for (int c = tid; c < k; c += 256) {
                int n = 0;
                for (int g = 0; g < n_part; ++g) n += part_i[(int64_t)g * is + c];
                counts[c] = n;
            }
        double sl = 0.0;
        for (int g = tid; g < n_part; g += 256) sl += (double)part_f[(int64_t)g * fs + kd] + (double)part_f[(int64_t)g * fs + kd + 1];
        shd[tid] = sl;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) shd[tid] += shd[tid + w];
            __syncthreads();
        }
        if (tid == 0) {
            *inertia = shd[0];
            if (stop) {
                ctl[1] = converged ? 1 : 0;
                ctl[0] = t;
            }
        }
        return;
    }
    const int jc = tid % KM_RED_COLS, sl = tid / KM_RED_COLS;
    const int64_t j = (int64_t)blockIdx.x * KM_RED_COLS + jc;
    const int per = (n_part + KM_RED_SLICES - 1) / KM_RED_SLICES;
    float s = 0.f;
    int n = 0;
    if (j < kd) {
        const int c = (int)(j / d);
        for (int g = sl * per; g < min(n_part, (sl + 1) * per); ++g) {
            s += part_f[(int64_t)g * fs + j];
            n += part_i[(int64_t)g * is + c];
        }
    }
    sh[tid] = s;
    shi[tid] = n;
    __syncthreads();
    if (sl == 0 && j < kd) {
        float ts = 0.f;
        int tn = 0;
        for (int q = 0; q < KM_RED_SLICES; ++q) {
            ts += sh[q * KM_RED_COLS + jc];
            tn += shi[q * KM_RED_COLS + jc];
        }
        sums[j] = ts;
        if (apply && tn > 0) cen[j] = ts / (float)tn;
    }
}

// cen[c][j] = E[ids[c]][j]: centroids given as node ids never visit the host
__global__ __launch_bounds__(256) void km_gather_kernel(const float *E, int ld, int d, const int32_t *ids, int k, float *cen) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= k * d) return;
    const int c = i / d, j = i - c * d;
    cen[i] = E[(int64_t)ids[c] * ld + j];
}

typedef void (*KmFn)(KmArgs);
#define KM_ROW(ct, s) {km_sweep_kernel<ct, 1, s>, km_sweep_kernel<ct, 2, s>, km_sweep_kernel<ct, 3, s>, km_sweep_kernel<ct, 4, s>, \
                       km_sweep_kernel<ct, 5, s>, km_sweep_kernel<ct, 6, s>, km_sweep_kernel<ct, 7, s>, km_sweep_kernel<ct, 8, s>}
// [0]: assign only, [1]: with the sums and counts
const KmFn km_sweeps[2][4][8] = {{KM_ROW(1, false), KM_ROW(2, false), KM_ROW(3, false), KM_ROW(4, false)},
                                 {KM_ROW(1, true), KM_ROW(2, true), KM_ROW(3, true), KM_ROW(4, true)}};

// The launch plan of a sweep (row_tiles.h) with its template instance
struct KmPlan : RowTilePlan {
    KmFn fn;
};

KmPlan km_plan(int64_t m, int k, int ld, bool with_sums) {
    const RowTilePlan t = row_tile_plan(m, k, ld);
    return KmPlan{t, km_sweeps[with_sums ? 1 : 0][t.CT - 1][t.DT - 1]};
}

// device state of a step or fit call
struct KmState {
    ScopedBuf nodes, ids, cen, part_f, part_i, sums, counts, inertia, ctl, assign, dist2;
};

int km_check(gg_ctx *ctx, const char *fn, int which, const int32_t *nodes, int64_t m, int k) {
    return check_rows(ctx, fn, which, nodes, m, [&] {
        GG_CHECK(ctx, k >= 1 && k <= RT_MAX_OUT, GG_EINVAL, "%s: k = %d outside [1, %d]", fn, k, RT_MAX_OUT);
        return (int)GG_OK;
    });
}

int km_check_ids(gg_ctx *ctx, const char *fn, const char *name, const int32_t *ids, int k) {
    for (int c = 0; c < k; ++c)
        GG_CHECK(ctx, ids[c] >= 0 && ids[c] < ctx->n_node, GG_EINVAL, "%s: %s[%d] = %d outside [0, %d)", fn, name, c, ids[c], ctx->n_node);
    return GG_OK;
}

// allocations (all before the first copy), the rows and the starting centroids (values, or table rows by id) on the device
hipError_t km_upload(gg_ctx *ctx, KmState &s, const KmPlan &p, int which, const int32_t *nodes, int64_t m, int k, const float *cen, const int32_t *ids,
                     bool want_assign, bool want_dist2, int n_inertia) {
    const int d = ctx->n_emb;
    const size_t kd = (size_t)k * d;
    hipError_t e = s.nodes.reserve(sizeof(int32_t) * m);
    if (e == hipSuccess) e = s.cen.reserve(sizeof(float) * kd);
    if (e == hipSuccess && ids) e = s.ids.reserve(sizeof(int32_t) * k);
    if (e == hipSuccess) e = s.part_f.reserve(sizeof(float) * (kd + 2) * p.grid);
    if (e == hipSuccess) e = s.part_i.reserve(sizeof(int32_t) * (size_t)(k + 1) * p.grid);
    if (e == hipSuccess) e = s.sums.reserve(sizeof(float) * kd);
    if (e == hipSuccess) e = s.counts.reserve(sizeof(int32_t) * k);
    if (e == hipSuccess) e = s.inertia.reserve(sizeof(double) * n_inertia);
    if (e == hipSuccess) e = s.ctl.reserve(sizeof(int32_t) * 2);
    if (e == hipSuccess && want_assign) e = s.assign.reserve(sizeof(int32_t) * m);
    if (e == hipSuccess && want_dist2) e = s.dist2.reserve(sizeof(float) * m);
    if (e == hipSuccess) e = hipMemcpyAsync(s.nodes.p, nodes, sizeof(int32_t) * m, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.ctl.p, 0, sizeof(int32_t) * 2, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s.part_i.p, 0, sizeof(int32_t) * (size_t)(k + 1) * p.grid, ctx->stream);
    if (e == hipSuccess && ids) {
        e = hipMemcpyAsync(s.ids.p, ids, sizeof(int32_t) * k, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess)
            hipLaunchKernelGGL(km_gather_kernel, dim3(cdiv(kd, 256)), dim3(256), 0, ctx->stream, ctx->model[which].E, ctx->ld, d, s.ids.as<int32_t>(), k,
                               s.cen.as<float>());
    } else if (e == hipSuccess) {
        e = hipMemcpyAsync(s.cen.p, cen, sizeof(float) * kd, hipMemcpyHostToDevice, ctx->stream);
    }
    if (e == hipSuccess && p.lds > 48 * 1024) e = hipFuncSetAttribute((const void *)p.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
    return e;
}

// sweep t + its update on ctx->stream (max_iters = 0: the totals alone, no update, no stop rule)
void km_enqueue(gg_ctx *ctx, const KmState &s, const KmPlan &p, bool with_sums, int which, int64_t m, int k, int t, int max_iters, double *inertia_dev) {
    const int d = ctx->n_emb;
    KmArgs a{ctx->model[which].E, s.nodes.as<int32_t>(), m, ctx->ld, d, k, s.cen.as<float>(), p.KW, s.part_f.as<float>(), s.part_i.as<int32_t>(),
             s.assign.as<int32_t>(), s.dist2.as<float>(), t > 1 ? 1 : 0, s.ctl.as<int32_t>(), t};
    hipLaunchKernelGGL(p.fn, dim3(p.grid), dim3(256), p.lds, ctx->stream, a);
    hipLaunchKernelGGL(km_update_kernel, dim3(with_sums ? cdiv((int64_t)k * d, KM_RED_COLS) + 1 : 1), dim3(256), 0, ctx->stream, s.part_f.as<float>(),
                       s.part_i.as<int32_t>(), p.grid, k, d, with_sums ? 1 : 0, s.cen.as<float>(), s.sums.as<float>(), s.counts.as<int32_t>(), inertia_dev,
                       s.ctl.as<int32_t>(), t, max_iters);
}

int step_call(gg_ctx *ctx, int which, const int32_t *nodes, int64_t m, int k, const float *centroids, const int32_t *centroid_nodes, int32_t *assign_out,
              float *dist2_out, float *sums_out, int32_t *counts_out, double *inertia_out) {
    const char *fn = "gg_kmeans_step";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (const int rc = km_check(ctx, fn, which, nodes, m, k)) return rc;
    GG_CHECK(ctx, (centroids != nullptr) != (centroid_nodes != nullptr), GG_EINVAL, "%s: exactly one of centroids and centroid_nodes must be given (got %s)",
             fn, centroids ? "both" : "neither");
    if (centroid_nodes)
        if (const int rc = km_check_ids(ctx, fn, "centroid_nodes", centroid_nodes, k)) return rc;
    GG_HIP(ctx, hipSetDevice(ctx->device));
    const size_t kd = (size_t)k * ctx->n_emb;
    const bool with_sums = sums_out || counts_out;
    const KmPlan p = km_plan(m, k, ctx->ld, with_sums);
    KmState s;
    GG_HIP_FN(km_upload(ctx, s, p, which, nodes, m, k, centroids, centroid_nodes, assign_out != nullptr, dist2_out != nullptr, 1));
    km_enqueue(ctx, s, p, with_sums, which, m, k, 1, 0, s.inertia.as<double>());
    GG_HIP_FN(hipGetLastError());
    if (assign_out) GG_HIP_FN(hipMemcpyAsync(assign_out, s.assign.p, sizeof(int32_t) * m, hipMemcpyDeviceToHost, ctx->stream));
    if (dist2_out) GG_HIP_FN(hipMemcpyAsync(dist2_out, s.dist2.p, sizeof(float) * m, hipMemcpyDeviceToHost, ctx->stream));
    if (sums_out) GG_HIP_FN(hipMemcpyAsync(sums_out, s.sums.p, sizeof(float) * kd, hipMemcpyDeviceToHost, ctx->stream));
    if (counts_out) GG_HIP_FN(hipMemcpyAsync(counts_out, s.counts.p, sizeof(int32_t) * k, hipMemcpyDeviceToHost, ctx->stream));
    if (inertia_out) GG_HIP_FN(hipMemcpyAsync(inertia_out, s.inertia.p, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipStreamSynchronize(ctx->stream));
    return GG_OK;
}

int fit_call(gg_ctx *ctx, int which, const int32_t *nodes, int64_t m, int k, int max_iters, float *centroids_inout, const int32_t *init_nodes,
             int32_t *assign_out, float *dist2_out, int32_t *counts_out, double *inertia_out, int32_t *iters_out, int32_t *converged_out, double *ms_out) {
    const char *fn = "gg_kmeans_fit";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (const int rc = km_check(ctx, fn, which, nodes, m, k)) return rc;
    GG_CHECK(ctx, max_iters >= 1 && max_iters <= 1000000, GG_EINVAL, "%s: max_iters = %d outside [1, 1000000]", fn, max_iters);
    GG_CHECK(ctx, centroids_inout != nullptr, GG_EINVAL, "%s: centroids_inout is NULL", fn);
    if (init_nodes)
        if (const int rc = km_check_ids(ctx, fn, "init_nodes", init_nodes, k)) return rc;
    GG_HIP(ctx, hipSetDevice(ctx->device));
    const size_t kd = (size_t)k * ctx->n_emb;
    const KmPlan p = km_plan(m, k, ctx->ld, true);
    KmState s;
    GG_HIP_FN(km_upload(ctx, s, p, which, nodes, m, k, centroids_inout, init_nodes, true, dist2_out != nullptr, max_iters));
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    for (int t = 1; t <= max_iters; ++t) km_enqueue(ctx, s, p, true, which, m, k, t, max_iters, s.inertia.as<double>() + (t - 1));
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    GG_HIP_FN(hipGetLastError());
    int32_t ctl[2] = {0, 0};
    GG_HIP_FN(hipMemcpyAsync(ctl, s.ctl.p, sizeof(ctl), hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipMemcpyAsync(centroids_inout, s.cen.p, sizeof(float) * kd, hipMemcpyDeviceToHost, ctx->stream));
    if (assign_out) GG_HIP_FN(hipMemcpyAsync(assign_out, s.assign.p, sizeof(int32_t) * m, hipMemcpyDeviceToHost, ctx->stream));
    if (dist2_out) GG_HIP_FN(hipMemcpyAsync(dist2_out, s.dist2.p, sizeof(float) * m, hipMemcpyDeviceToHost, ctx->stream));
    if (counts_out) GG_HIP_FN(hipMemcpyAsync(counts_out, s.counts.p, sizeof(int32_t) * k, hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipStreamSynchronize(ctx->stream));
    GG_CHECK(ctx, ctl[0] >= 1 && ctl[0] <= max_iters, GG_EHIP, "%s: the device reported %d sweeps of at most %d", fn, ctl[0], max_iters);
    if (inertia_out) {  // the sweeps that ran; later entries are not written
        GG_HIP_FN(hipMemcpyAsync(inertia_out, s.inertia.p, sizeof(double) * ctl[0], hipMemcpyDeviceToHost, ctx->stream));
        GG_HIP_FN(hipStreamSynchronize(ctx->stream));
    }
    if (iters_out) *iters_out = ctl[0];
    if (converged_out) *converged_out = ctl[1];
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    if (ms_out) *ms_out = ms;
    return GG_OK;
}

}  // namespace

}  // namespace gg

using namespace gg;

// gg_kmeans_step, gg_kmeans_fit: see include/graphgan_hip.h.
extern "C" int gg_kmeans_step(gg_ctx *ctx, int which, const int32_t *nodes, int64_t m, int k, const float *centroids, const int32_t *centroid_nodes,
                              int32_t *assign_out, float *dist2_out, float *sums_out, int32_t *counts_out, double *inertia_out) {
    return step_call(ctx, which, nodes, m, k, centroids, centroid_nodes, assign_out, dist2_out, sums_out, counts_out, inertia_out);
}

extern "C" int gg_kmeans_fit(gg_ctx *ctx, int which, const int32_t *nodes, int64_t m, int k, int max_iters, float *centroids_inout,
                             const int32_t *init_nodes, int32_t *assign_out, float *dist2_out, int32_t *counts_out, double *inertia_out,
                             int32_t *iters_out, int32_t *converged_out, double *ms_out) {
    return fit_call(ctx, which, nodes, m, k, max_iters, centroids_inout, init_nodes, assign_out, dist2_out, counts_out, inertia_out, iters_out,
                    converged_out, ms_out);
}
