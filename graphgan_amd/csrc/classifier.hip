// classifier.hip -- node classification: multinomial logistic regression on rows of a resident table, gathered by node id.
//     z = W . E[node] + b                         W fp32 [C, d], b fp32 [C]
//     loss = -(1/M) sum log softmax(z)[label] + (l2 / 2) |W|^2            (the bias is not regularised)
//     gW = (1/M) sum (p - onehot) E[node]^T + l2 W,   gb = (1/M) sum (p - onehot)
// nc_sweep_kernel is the hot path: ONE sweep over the M rows gives the loss and both gradients.  It is the row-tile sweep of
// row_tiles.h (gather, logits Z = Xs . W^T, row stage, gradient G += P^T . Xs; the geometry, the barriers and the launch plan
// are described there) with this file's row stage: a max-subtracted softmax per row in LDS (4 threads per row), the row's loss
// term, P = p - onehot left in LDS; gb += column sums of P.
// Every workgroup writes its partial [C d + C + 2] (gW, gb, the float64 loss as two floats) to a stage and nc_reduce_kernel sums
// the stage in a fixed order.  No floating-point atomics anywhere: two calls with the same inputs give the same bits.
// nc_adam_kernel: full-batch Adam on (W, b); nc_predict_kernel: logits + argmax (ties to the lowest class).
//
// Multi-label (gg_classifier_ml_*): one-vs-rest logistic regression against a multi-hot mask uint32 [M][CT] (bit c & 31 of word
// c >> 5 = row has class c):
//     loss = (1/M) sum_i sum_c [softplus(z_ic) - y_ic z_ic] + (l2 / 2) |W|^2,   gW = (1/M) sum (sigmoid(z) - y) E[node]^T + l2 W
// It is the SAME sweep with a second compile-time variant of the row stage (template parameter ML; everything else, the stage,
// nc_reduce_kernel and nc_adam_kernel are shared): per class, with e = exp(-|z|), softplus(z) = max(z, 0) + log1p(e) and
// sigmoid(z) = (z >= 0 ? 1 : e) / (1 + e) -- finite at any logit, and exactly 0 or 1 once e underflows.
// nc_ml_predict_kernel: logits, the rank of every class in (logit descending, class ascending) and the mask of the first k[i]
// classes of that order (or of the classes with z > 0).
#include <math.h>

#include <algorithm>
#include <vector>

#include "row_tiles.h"

namespace gg {

namespace {

constexpr int NC_RED_COLS = 32, NC_RED_SLICES = 8;  // nc_reduce_kernel: columns x stage slices per workgroup

struct SweepArgs {
    const float *E;          // [n_node, ld]
    const int32_t *nodes, *labels;  // labels: one class per row (softmax variant)
    int64_t m;
    int ld, d, C;
    const float *W, *b;      // [C, d], [C]
    int KW;                  // k-chunk of the W staging (>= ld: W is staged once)
    float *part;             // [grid][C d + C + 2]: gW, gb, the loss as (high, remainder)
    const uint32_t *bits;    // [m][CT] multi-hot label mask (sigmoid variant)
};

template <int CT, int DT, bool ML>
__global__ __launch_bounds__(256) void nc_sweep_kernel(SweepArgs a) {
    constexpr int PS = RowTiles<CT, DT>::PS;
    extern __shared__ float nc_lds[];
    __shared__ float bs[RT_MAX_OUT];  // the bias
    __shared__ double red[256];  // the workgroup's loss terms (float64: a sum of M terms of size log C must keep the last digits)
    const int tid = threadIdx.x, d = a.d, C = a.C;
    double loss_acc = 0.0;
    float gb_acc = 0.f;

    auto setup = [&](const float *, int, bool) {
        if (tid < C) bs[tid] = a.b[tid];
    };
    // the per-row loss stage of row tid >> 2 by 4 threads (classes q, q + 4, ...); P is zero for rows behind M and padded classes
    auto rows = [&](int64_t row0, const float *, float *Ps) {
        if constexpr (ML) {
            // per-class sigmoid cross-entropy against the row's mask words (word j holds classes 32 j .. 32 j + 31; CT words per
            // row); P = sigmoid(z) - y.  No row maximum, nothing crosses lanes.
            const int r = tid >> 2, q = tid & 3;
            const bool valid = row0 + r < a.m;
            float *p = Ps + r * PS;
#pragma unroll
            for (int j = 0; j < CT; ++j) {
                const uint32_t yw = valid ? a.bits[(row0 + r) * CT + j] : 0u;
                const int c_end = min(C, 32 * j + 32);
                for (int c = 32 * j + q; c < c_end; c += 4) {
                    const float z = p[c] + bs[c];
                    const bool y = (yw >> (c & 31)) & 1u;
                    const float e = expf(-fabsf(z));
                    const float sg = (z >= 0.f ? 1.f : e) / (1.f + e);
                    if (valid) loss_acc += (double)(fmaxf(z, 0.f) + log1pf(e)) - (y ? (double)z : 0.0);
                    p[c] = valid ? sg - (y ? 1.f : 0.f) : 0.f;
                }
            }
            for (int c = C + q; c < 32 * CT; c += 4) p[c] = 0.f;
        } else {
            // max-subtracted softmax; P = p - onehot
            const int r = tid >> 2, q = tid & 3;
            const bool valid = row0 + r < a.m;
            const int lab = valid ? a.labels[row0 + r] : -1;
            float *p = Ps + r * PS;
            float mx = -INFINITY, zl = 0.f;  // zl: the label's logit (held by the thread that owns the label's class)
            for (int c = q; c < C; c += 4) {
                const float z = p[c] + bs[c];
                p[c] = z;
                mx = fmaxf(mx, z);
                zl = c == lab ? z : zl;
            }
            mx = fmaxf(mx, __shfl_xor(mx, 1));
            mx = fmaxf(mx, __shfl_xor(mx, 2));
            float s = 0.f;
            for (int c = q; c < C; c += 4) {  // (one exponential per class: it is kept in place of the logit)
                const float e = expf(p[c] - mx);
                p[c] = e;
                s += e;
            }
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            const float inv = 1.f / s;
            if (lab >= 0 && (lab & 3) == q) loss_acc += (double)((logf(s) + mx) - zl);
            for (int c = q; c < C; c += 4) {
                const float g = p[c] * inv - (c == lab ? 1.f : 0.f);
                p[c] = valid ? g : 0.f;
            }
            for (int c = C + q; c < 32 * CT; c += 4) p[c] = 0.f;
        }
    };
    auto column = [&](float p) { gb_acc += p; };  // (a float sum with r ascending)
    // the workgroup's partial: gW [C, d], gb [C], loss (two floats)
    float *part = a.part + (int64_t)blockIdx.x * ((int64_t)C * d + C + 2);
    row_tile_sweep<CT, DT, true>(nc_lds, a.E, a.nodes, a.m, a.ld, d, C, a.W, a.KW, part, setup, rows, column);
    if (tid < C) part[(int64_t)C * d + tid] = gb_acc;
    rt_block_sum(red, loss_acc, part + (int64_t)C * d + C);
}

// grad[j] = (1/M) sum_g part[g][j] (+ l2 W[j] for j < C d) for the C d + C gradient entries: a workgroup takes NC_RED_COLS
// entries, NC_RED_SLICES threads per entry sum contiguous slices of the stage, thread 0 of the entry adds the slices in order.
// The LAST workgroup gives the loss: (1/M) sum_g (part[g][C d + C] + part[g][C d + C + 1]) + (l2 / 2) |W|^2, both by strided
// sums and a fixed tree.
__global__ __launch_bounds__(256) void nc_reduce_kernel(const float *part, int n_part, int C, int d, int64_t m, const float *W, float l2,
                                                       float *grad, float *loss_out) {
    __shared__ float sh[256];
    __shared__ double shd[256];
    const int tid = threadIdx.x;
    const int64_t cd = (int64_t)C * d, n_out = cd + C, stride = n_out + 2;
    const float fm = (float)m;
    if (blockIdx.x == gridDim.x - 1) {
        double sl = 0.0;  // (the loss terms in float64, as in the sweep)
        float sw = 0.f;
        for (int g = tid; g < n_part; g += 256) sl += (double)part[(int64_t)g * stride + n_out] + (double)part[(int64_t)g * stride + n_out + 1];
        for (int64_t j = tid; j < cd; j += 256) sw += W[j] * W[j];
        shd[tid] = sl;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) shd[tid] += shd[tid + w];
            __syncthreads();
        }
        const double tl = shd[0];
        sh[tid] = sw;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) sh[tid] += sh[tid + w];
            __syncthreads();
        }
        if (tid == 0) {
            const float loss = (float)(tl / (double)m + (double)(0.5f * l2 * sh[0]));
            grad[n_out] = loss;
            if (loss_out) *loss_out = loss;
        }
        return;
    }
    const int jc = tid % NC_RED_COLS, sl = tid / NC_RED_COLS;
    const int64_t j = (int64_t)blockIdx.x * NC_RED_COLS + jc;
    const int per = (n_part + NC_RED_SLICES - 1) / NC_RED_SLICES;
    float s = 0.f;
    if (j < n_out)
        for (int g = sl * per; g < min(n_part, (sl + 1) * per); ++g) s += part[(int64_t)g * stride + j];
    sh[tid] = s;
    __syncthreads();
    if (sl == 0 && j < n_out) {
        float t = 0.f;
        for (int q = 0; q < NC_RED_SLICES; ++q) t += sh[q * NC_RED_COLS + jc];
        t /= fm;
        if (j < cd) t += l2 * W[j];
        grad[j] = t;
    }
}

// full-batch Adam on theta = (W, b): c1 = 1 - beta1^t, c2 = 1 - beta2^t of step t (from 1)
__global__ __launch_bounds__(256) void nc_adam_kernel(float *theta, float *mom, float *var, const float *grad, int64_t n, float lr, float c1, float c2) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const float g = grad[j];
    const float mj = 0.9f * mom[j] + (1.f - 0.9f) * g;
    const float vj = 0.999f * var[j] + (1.f - 0.999f) * (g * g);
    mom[j] = mj;
    var[j] = vj;
    theta[j] -= lr * (mj / c1) / (sqrtf(vj / c2) + 1e-8f);
}

// The front end of both prediction kernels.  One wavefront per row at a time: W in LDS ([C][ld + 1], zero padded), the row in
// LDS, lane c (and c + 64) the class's dot product.  What a kernel does with its logits is its own tail.
__device__ __forceinline__ void nc_stage_w(float *Ws, const float *W, int C, int d, int ld) {
    for (int i = threadIdx.x; i < C * ld; i += 256) {
        const int c = i / ld, kk = i - c * ld;
        Ws[c * (ld + 1) + kk] = kk < d ? W[(int64_t)c * d + kk] : 0.f;
    }
    __syncthreads();
}

// the wavefront's LDS writes (the staged row; a kernel's published logits) become visible to its other lanes; also behind the
// last read of a row, before the next one overwrites it
__device__ __forceinline__ void nc_wave_sync() {
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
}

__device__ __forceinline__ void nc_stage_row(float *xs, const float *x, int ld, int lane) {
    for (int kk = lane; kk < ld; kk += 64) xs[kk] = x[kk];
    nc_wave_sync();
}

// z[c] = sum_kk W[c][kk] x[kk] (kk ascending from 0: the order is part of the result) + b[c] of row `row`, stored to
// logits [m][C] if given
__device__ __forceinline__ float nc_logit(const float *Ws, const float *xs, int ld, const float *b, int c, float *logits, int64_t row, int C) {
    const float *w = Ws + c * (ld + 1);
    float z = 0.f;
    for (int kk = 0; kk < ld; ++kk) z += w[kk] * xs[kk];
    z += b[c];
    if (logits) logits[row * C + c] = z;
    return z;
}

// nc_ml_predict_kernel -- lane c holds the logits of classes c and c + 64 and publishes them to LDS (zs); every lane then
// counts, over all C published logits (one broadcast read each), the classes that come before its own in the total order
// (logit descending, class ascending): the rank.  A class is selected when rank < k[row] (k given) or z > 0 (k NULL).  Two
// ballots give the four mask words; lane j stores word j.
__global__ __launch_bounds__(256) void nc_ml_predict_kernel(const float *E, int ld, int d, const int32_t *nodes, int64_t m, int C, const float *W,
                                                           const float *b, const int32_t *k, uint32_t *pred_bits, float *logits) {
    extern __shared__ float nc_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, CW = (C + 31) >> 5;
    float *Ws = nc_lds, *xs = Ws + C * (ld + 1) + wv * ld, *zs = Ws + C * (ld + 1) + 4 * ld + wv * RT_MAX_OUT;
    nc_stage_w(Ws, W, C, d, ld);
    for (int64_t row = (int64_t)blockIdx.x * 4 + wv; row < m; row += (int64_t)gridDim.x * 4) {
        nc_stage_row(xs, E + (int64_t)nodes[row] * ld, ld, lane);
        float z0 = 0.f, z1 = 0.f;
        if (lane < C) zs[lane] = z0 = nc_logit(Ws, xs, ld, b, lane, logits, row, C);
        if (lane + 64 < C) zs[lane + 64] = z1 = nc_logit(Ws, xs, ld, b, lane + 64, logits, row, C);
        nc_wave_sync();
        bool sel0, sel1;
        if (k) {
            int rank0 = 0, rank1 = 0;
            for (int c = 0; c < C; ++c) {
                const float o = zs[c];
                rank0 += (o > z0 || (o == z0 && c < lane)) ? 1 : 0;
                rank1 += (o > z1 || (o == z1 && c < lane + 64)) ? 1 : 0;
            }
            const int kr = k[row];
            sel0 = lane < C && rank0 < kr;
            sel1 = lane + 64 < C && rank1 < kr;
        } else {
            sel0 = lane < C && z0 > 0.f;
            sel1 = lane + 64 < C && z1 > 0.f;
        }
        const unsigned long long m0 = __ballot(sel0), m1 = __ballot(sel1);  // classes 0 .. 63, 64 .. 127
        if (lane < CW) pred_bits[row * CW + lane] = (uint32_t)((lane < 2 ? m0 : m1) >> (32 * (lane & 1)));
        nc_wave_sync();
    }
}

// nc_predict_kernel -- argmax over (logit descending, class ascending) by a butterfly.
__global__ __launch_bounds__(256) void nc_predict_kernel(const float *E, int ld, int d, const int32_t *nodes, int64_t m, int C, const float *W,
                                                        const float *b, int32_t *pred, float *logits) {
    extern __shared__ float nc_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float *Ws = nc_lds, *xs = Ws + C * (ld + 1) + wv * ld;
    nc_stage_w(Ws, W, C, d, ld);
    for (int64_t row = (int64_t)blockIdx.x * 4 + wv; row < m; row += (int64_t)gridDim.x * 4) {
        nc_stage_row(xs, E + (int64_t)nodes[row] * ld, ld, lane);
        float best = -INFINITY;
        int bc = 0x7fffffff;
        for (int c = lane; c < C; c += 64) {
            const float z = nc_logit(Ws, xs, ld, b, c, logits, row, C);
            if (z > best || bc == 0x7fffffff) {  // (the lane's classes ascend: a later equal logit does not replace)
                best = z;
                bc = c;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o);
            const int oc = __shfl_xor(bc, o);
            if (oc != 0x7fffffff && (bc == 0x7fffffff || ob > best || (ob == best && oc < bc))) {
                best = ob;
                bc = oc;
            }
        }
        if (lane == 0) pred[row] = bc;
        nc_wave_sync();
    }
}

// ---- link prediction (gg_edge_classifier_*): logistic regression on a binary operator of the two endpoint rows of an edge
//     x_i = op(E[u_i], E[v_i]) elementwise,   z_i = w . x_i + b                     w fp32 [d], b fp32 [1]
//     loss = (1/M) sum [softplus(z_i) - y_i z_i] + (l2 / 2) |w|^2,   gw = (1/M) sum (sigmoid(z_i) - y_i) x_i + l2 w
// One logit per row: nothing for a matrix instruction to do, and the two random row gathers are all the work.
// edge_sweep_kernel is a persistent grid of min(EC_MAX_GRID, ceil(M / 16)) workgroups (a function of M alone); a trip of a
// workgroup is 16 edges, trips go to workgroups round robin.  EC_LANES = 16 lanes own an edge; lane l owns the float4 pieces
// l + 16 j (j < NJ = ceil(ld / 64), a template parameter) of both rows, of w and of the gw accumulator, all in registers across
// the workgroup's trips.  Memory-level parallelism: the rows of the NEXT trip (2 rows x NJ float4 per lane) are in flight
// while this one computes, and the ids of the trip after that are in flight behind them, so no row address waits for an id.
// The logit is a 4-step butterfly over the 16 lanes (every lane ends with the same bits).  The loss stage is the multi-label
// sweep's: e = exp(-|z|), softplus = max(z, 0) + log1p(e), sigmoid = (z >= 0 ? 1 : e) / (1 + e), the loss in float64.  Columns
// in [d, ld) and edges behind M give exact zeros.  At the end the 16 lane groups fold through LDS in group order and the
// workgroup writes part[blockIdx][d + 1 + 2] = gw, gb, loss (high, remainder): the stage nc_reduce_kernel reads at C = 1.  No
// floating-point atomics.  All four operators are symmetric in their operands bit for bit (a - b and b - a differ in sign alone).
constexpr int EC_LANES = 16;               // lanes per edge
constexpr int EC_EDGES = 256 / EC_LANES;   // edges of a trip
constexpr int EC_MAX_GRID = 1024;          // workgroups of an edge sweep, at most
constexpr int EC_PREDICT_GRID = 1024;      // workgroups of edge_predict_kernel, at most

struct EdgeArgs {
    const float *E;              // [n_node, ld]
    const int32_t *u, *v, *y;    // y: 0 | 1 (the sweep's alone)
    int64_t m;
    int ld, d;
    const float *w, *b;          // [d], [1]
    float *part;                 // sweep: [grid][d + 3]
    float *logits;               // predict: [m]
};

// 0 Hadamard, 1 average, 2 L1, 3 L2 (the node2vec paper's table)
template <int OP>
__device__ __forceinline__ float ec_op(float a, float b) {
    if constexpr (OP == 0) {
        return a * b;
    } else if constexpr (OP == 1) {
        return (a + b) * 0.5f;
    } else if constexpr (OP == 2) {
        return fabsf(a - b);
    } else {
        const float t = a - b;
        return t * t;
    }
}

// the lane's slice of w: pieces l + 16 j, zero behind d
template <int NJ>
__device__ __forceinline__ void ec_load_w(float4 (&w)[NJ], const float *wp, int l, int d) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = 4 * (l + EC_LANES * j);
        w[j].x = col < d ? wp[col] : 0.f;
        w[j].y = col + 1 < d ? wp[col + 1] : 0.f;
        w[j].z = col + 2 < d ? wp[col + 2] : 0.f;
        w[j].w = col + 3 < d ? wp[col + 3] : 0.f;
    }
}

// the lane's pieces of both rows of an edge (zeros for an edge behind M and for pieces behind ld)
template <int NJ>
__device__ __forceinline__ void ec_fetch(float4 (&ra)[NJ], float4 (&rb)[NJ], const float *E, int iu, int iv, bool ok, int l, int ld) {
    const float *pa = E + (int64_t)iu * ld, *pb = E + (int64_t)iv * ld;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = 4 * (l + EC_LANES * j);
        ra[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        rb[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok && col < ld) {
            ra[j] = *(const float4 *)(pa + col);
            rb[j] = *(const float4 *)(pb + col);
        }
    }
}

// x = op(ra, rb) (left in ra; columns behind d: 0) and w . x summed over the edge's 16 lanes: every lane returns the same bits
template <int OP, int NJ>
__device__ __forceinline__ float ec_features(float4 (&ra)[NJ], const float4 (&rb)[NJ], const float4 (&w)[NJ], int l, int d) {
    float z = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = 4 * (l + EC_LANES * j);
        float4 x;
        x.x = col < d ? ec_op<OP>(ra[j].x, rb[j].x) : 0.f;
        x.y = col + 1 < d ? ec_op<OP>(ra[j].y, rb[j].y) : 0.f;
        x.z = col + 2 < d ? ec_op<OP>(ra[j].z, rb[j].z) : 0.f;
        x.w = col + 3 < d ? ec_op<OP>(ra[j].w, rb[j].w) : 0.f;
        ra[j] = x;
        z += w[j].x * x.x;
        z += w[j].y * x.y;
        z += w[j].z * x.z;
        z += w[j].w * x.w;
    }
#pragma unroll
    for (int o = EC_LANES / 2; o > 0; o >>= 1) z += __shfl_xor(z, o);
    return z;
}

template <int OP, int NJ>
__global__ __launch_bounds__(256) void edge_sweep_kernel(EdgeArgs a) {
    __shared__ float gs[EC_EDGES][RT_MAX_D];  // the lane groups' gw
    __shared__ float gbs[EC_EDGES];
    __shared__ double ls[EC_EDGES];
    const int tid = threadIdx.x, g = tid / EC_LANES, l = tid % EC_LANES;
    const int ld = a.ld, d = a.d;
    const int64_t n_trips = (a.m + EC_EDGES - 1) / EC_EDGES;

    float4 w[NJ], gw[NJ];
    ec_load_w<NJ>(w, a.w, l, d);
#pragma unroll
    for (int j = 0; j < NJ; ++j) gw[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float bias = a.b[0];
    double loss_acc = 0.0;
    float gb_acc = 0.f;

    int iu = 0, iv = 0, iy = 0;  // the ids and the label of the trip after the next
    bool ok = false;
    auto load_ids = [&](int64_t trip) {  // (a trip behind the last one has every edge behind M)
        const int64_t e = trip * EC_EDGES + g;
        ok = e < a.m;
        iu = ok ? a.u[e] : 0;
        iv = ok ? a.v[e] : 0;
        iy = ok ? a.y[e] : 0;
    };
    float4 na[NJ], nb[NJ];  // the next trip's rows
    int ny = 0;
    bool nok = false;

    load_ids(blockIdx.x);
    ec_fetch<NJ>(na, nb, a.E, iu, iv, ok, l, ld);
    ny = iy;
    nok = ok;
    load_ids((int64_t)blockIdx.x + gridDim.x);
    for (int64_t trip = blockIdx.x; trip < n_trips; trip += gridDim.x) {
        float4 ca[NJ], cb[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            ca[j] = na[j];
            cb[j] = nb[j];
        }
        const int cy = ny;
        const bool cok = nok;
        ec_fetch<NJ>(na, nb, a.E, iu, iv, ok, l, ld);
        ny = iy;
        nok = ok;
        load_ids(trip + 2 * (int64_t)gridDim.x);

        const float z = ec_features<OP, NJ>(ca, cb, w, l, d) + bias;
        const float e = expf(-fabsf(z));
        const float sg = (z >= 0.f ? 1.f : e) / (1.f + e);
        const float p = cok ? sg - (float)cy : 0.f;
        if (l == 0) {
            if (cok) loss_acc += (double)(fmaxf(z, 0.f) + log1pf(e)) - (cy ? (double)z : 0.0);
            gb_acc += p;
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            gw[j].x += p * ca[j].x;
            gw[j].y += p * ca[j].y;
            gw[j].z += p * ca[j].z;
            gw[j].w += p * ca[j].w;
        }
    }

    // the workgroup's partial: the 16 lane groups in group order
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = 4 * (l + EC_LANES * j);
        if (col < ld) *(float4 *)&gs[g][col] = gw[j];
    }
    if (l == 0) {
        gbs[g] = gb_acc;
        ls[g] = loss_acc;
    }
    __syncthreads();
    float *part = a.part + (int64_t)blockIdx.x * (d + 3);
    if (tid < d) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < EC_EDGES; ++q) s += gs[q][tid];
        part[tid] = s;
    }
    if (tid == 0) {
        float sb = 0.f;
        double sl = 0.0;
        for (int q = 0; q < EC_EDGES; ++q) {
            sb += gbs[q];
            sl += ls[q];
        }
        const float hi = (float)sl;
        part[d] = sb;
        part[d + 1] = hi;
        part[d + 2] = (float)(sl - (double)hi);
    }
}

// edge_predict_kernel: logits[i] = w . op(E[u_i], E[v_i]) + b by the sweep's gather, operator and butterfly (the same bits as
// the sweep's logit); nothing is summed across edges.  Trips of 16 edges go to min(EC_PREDICT_GRID, ceil(M / 16)) workgroups
// round robin.
template <int OP, int NJ>
__global__ __launch_bounds__(256) void edge_predict_kernel(EdgeArgs a) {
    const int tid = threadIdx.x, g = tid / EC_LANES, l = tid % EC_LANES;
    const int64_t n_trips = (a.m + EC_EDGES - 1) / EC_EDGES;
    float4 w[NJ];
    ec_load_w<NJ>(w, a.w, l, a.d);
    const float bias = a.b[0];
    for (int64_t trip = blockIdx.x; trip < n_trips; trip += gridDim.x) {
        const int64_t e = trip * EC_EDGES + g;
        const bool ok = e < a.m;
        float4 ra[NJ], rb[NJ];
        ec_fetch<NJ>(ra, rb, a.E, ok ? a.u[e] : 0, ok ? a.v[e] : 0, ok, l, a.ld);
        const float z = ec_features<OP, NJ>(ra, rb, w, l, a.d) + bias;
        if (ok && l == 0) a.logits[e] = z;
    }
}

typedef void (*EdgeFn)(EdgeArgs);
#define EC_ROW(k, op) {k<op, 1>, k<op, 2>, k<op, 3>, k<op, 4>}
const EdgeFn ec_sweeps[4][4] = {EC_ROW(edge_sweep_kernel, 0), EC_ROW(edge_sweep_kernel, 1), EC_ROW(edge_sweep_kernel, 2), EC_ROW(edge_sweep_kernel, 3)};
const EdgeFn ec_predicts[4][4] = {EC_ROW(edge_predict_kernel, 0), EC_ROW(edge_predict_kernel, 1), EC_ROW(edge_predict_kernel, 2),
                                  EC_ROW(edge_predict_kernel, 3)};

typedef void (*SweepFn)(SweepArgs);
#define NC_ROW(ct, ml) {nc_sweep_kernel<ct, 1, ml>, nc_sweep_kernel<ct, 2, ml>, nc_sweep_kernel<ct, 3, ml>, nc_sweep_kernel<ct, 4, ml>, \
                        nc_sweep_kernel<ct, 5, ml>, nc_sweep_kernel<ct, 6, ml>, nc_sweep_kernel<ct, 7, ml>, nc_sweep_kernel<ct, 8, ml>}
// [0]: softmax against one class per row, [1]: per-class sigmoid against a multi-hot mask
const SweepFn nc_sweeps[2][4][8] = {{NC_ROW(1, false), NC_ROW(2, false), NC_ROW(3, false), NC_ROW(4, false)},
                                    {NC_ROW(1, true), NC_ROW(2, true), NC_ROW(3, true), NC_ROW(4, true)}};

// The launch plan of a sweep (row_tiles.h) with its template instance
struct SweepPlan : RowTilePlan {
    SweepFn fn;
};

SweepPlan sweep_plan(int64_t m, int C, int ld, bool ml) {
    const RowTilePlan t = row_tile_plan(m, C, ld);
    return SweepPlan{t, nc_sweeps[ml ? 1 : 0][t.CT - 1][t.DT - 1]};
}

// device state of an Adam fit (adam_fit); theta = (W, b)
struct AdamBufs {
    ScopedBuf theta, mom, var, grad, loss;
};

// device state of a fit or loss-and-gradient call
struct Fit : AdamBufs {
    ScopedBuf nodes, labels, part;
};

int check_common(gg_ctx *ctx, const char *fn, int which, const int32_t *nodes, int64_t m, int n_class) {
    return check_rows(ctx, fn, which, nodes, m, [&] {
        GG_CHECK(ctx, n_class >= 2 && n_class <= RT_MAX_OUT, GG_EINVAL, "%s: n_class = %d outside [2, %d]", fn, n_class, RT_MAX_OUT);
        return (int)GG_OK;
    });
}

int check_labels(gg_ctx *ctx, const char *fn, const int32_t *labels, int64_t m, int n_class) {
    GG_CHECK(ctx, labels != nullptr, GG_EINVAL, "%s: labels is NULL", fn);
    for (int64_t i = 0; i < m; ++i)
        GG_CHECK(ctx, labels[i] >= 0 && labels[i] < n_class, GG_EINVAL, "%s: label %d (entry %lld) outside [0, n_class = %d)", fn, labels[i], (long long)i, n_class);
    return GG_OK;
}

// multi-hot masks [m][CW]: no bit at a position >= n_class
int check_label_bits(gg_ctx *ctx, const char *fn, const uint32_t *bits, int64_t m, int n_class) {
    GG_CHECK(ctx, bits != nullptr, GG_EINVAL, "%s: label_bits is NULL", fn);
    const int CW = cdiv(n_class, 32), tail = n_class & 31;
    if (tail == 0) return GG_OK;
    const uint32_t stray = ~0u << tail;
    for (int64_t i = 0; i < m; ++i) {
        const uint32_t w = bits[i * CW + CW - 1] & stray;
        GG_CHECK(ctx, w == 0, GG_EINVAL, "%s: label_bits row %lld has bit %d set, outside [0, n_class = %d)", fn, (long long)i,
                 32 * (CW - 1) + __builtin_ctz(w), n_class);
    }
    return GG_OK;
}

// the rows and the parameters of a call to the device: nodes int32 [m], theta = (W [C, d], b [C]).  The caller has reserved both,
// with its other buffers: every allocation of a call comes before its first copy.
hipError_t upload_nodes_theta(gg_ctx *ctx, DevBuf &d_nodes, DevBuf &d_theta, const int32_t *nodes, int64_t m, int C, const float *W, const float *b) {
    const size_t cd = (size_t)C * ctx->n_emb;
    hipError_t e = hipMemcpyAsync(d_nodes.p, nodes, sizeof(int32_t) * m, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_theta.p, W, sizeof(float) * cd, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_theta.as<float>() + cd, b, sizeof(float) * C, hipMemcpyHostToDevice, ctx->stream);
    return e;
}

// nodes, labels (one int32 class per row, or with `ml` the mask words uint32 [m][ceil(C / 32)]), theta = (W, b) on the device;
// the stage and the gradient
hipError_t fit_upload(gg_ctx *ctx, Fit &f, const SweepPlan &p, bool ml, const int32_t *nodes, const void *labels, int64_t m, int C, const float *W,
                      const float *b) {
    const size_t n_par = (size_t)C * ctx->n_emb + C;
    const size_t label_bytes = sizeof(int32_t) * (size_t)m * (ml ? cdiv(C, 32) : 1);
    hipError_t e = f.nodes.reserve(sizeof(int32_t) * m);
    if (e == hipSuccess) e = f.labels.reserve(label_bytes);
    if (e == hipSuccess) e = f.theta.reserve(sizeof(float) * n_par);
    if (e == hipSuccess) e = f.grad.reserve(sizeof(float) * (n_par + 1));
    if (e == hipSuccess) e = f.part.reserve(sizeof(float) * (n_par + 2) * p.grid);
    if (e == hipSuccess) e = upload_nodes_theta(ctx, f.nodes, f.theta, nodes, m, C, W, b);
    if (e == hipSuccess) e = hipMemcpyAsync(f.labels.p, labels, label_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && p.lds > 48 * 1024) e = hipFuncSetAttribute((const void *)p.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
    return e;
}

// sweep + reduce of theta on ctx->stream: grad [C d + C + 1] (the loss last), the loss also to *loss_dev
void enqueue_lossgrad(gg_ctx *ctx, const Fit &f, const SweepPlan &p, int which, int64_t m, int C, float l2, float *loss_dev) {
    const int d = ctx->n_emb;
    const int64_t cd = (int64_t)C * d;
    SweepArgs a{ctx->model[which].E, f.nodes.as<int32_t>(), f.labels.as<int32_t>(), m, ctx->ld, d, C, f.theta.as<float>(), f.theta.as<float>() + cd, p.KW,
                f.part.as<float>(), f.labels.as<uint32_t>()};
    hipLaunchKernelGGL(p.fn, dim3(p.grid), dim3(256), p.lds, ctx->stream, a);
    hipLaunchKernelGGL(nc_reduce_kernel, dim3(cdiv(cd + C, NC_RED_COLS) + 1), dim3(256), 0, ctx->stream, f.part.as<float>(), p.grid, C, d, m,
                       f.theta.as<float>(), l2, f.grad.as<float>(), loss_dev);
}

// the labels of either variant: `ml` false -- one class per row, true -- the mask words
int check_any_labels(gg_ctx *ctx, const char *fn, bool ml, const void *labels, int64_t m, int n_class) {
    return ml ? check_label_bits(ctx, fn, (const uint32_t *)labels, m, n_class) : check_labels(ctx, fn, (const int32_t *)labels, m, n_class);
}

// gg_classifier_lossgrad / gg_classifier_ml_lossgrad (fn names the entry point in the error texts)
int lossgrad_call(gg_ctx *ctx, const char *fn, bool ml, int which, const int32_t *nodes, const void *labels, int64_t m, int n_class, const float *W,
                  const float *b, float l2, float *loss_out, float *gW_out, float *gb_out) {
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (const int rc = check_common(ctx, fn, which, nodes, m, n_class)) return rc;
    if (const int rc = check_any_labels(ctx, fn, ml, labels, m, n_class)) return rc;
    GG_CHECK(ctx, W && b && loss_out && gW_out && gb_out, GG_EINVAL, "%s: W, b, loss_out, gW_out, gb_out must not be NULL", fn);
    GG_CHECK(ctx, l2 >= 0.f && std::isfinite(l2), GG_EINVAL, "%s: l2 must be finite and >= 0", fn);
    GG_HIP(ctx, hipSetDevice(ctx->device));
    const int C = n_class;
    const size_t cd = (size_t)C * ctx->n_emb;
    const SweepPlan p = sweep_plan(m, C, ctx->ld, ml);
    Fit f;
    GG_HIP_FN(fit_upload(ctx, f, p, ml, nodes, labels, m, C, W, b));
    enqueue_lossgrad(ctx, f, p, which, m, C, l2, nullptr);
    GG_HIP_FN(hipGetLastError());
    GG_HIP_FN(hipMemcpyAsync(gW_out, f.grad.p, sizeof(float) * cd, hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipMemcpyAsync(gb_out, f.grad.as<float>() + cd, sizeof(float) * C, hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipMemcpyAsync(loss_out, f.grad.as<float>() + cd + C, sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipStreamSynchronize(ctx->stream));
    return GG_OK;
}

// `iters` steps of full-batch Adam on theta = (W [n_w], b [n_b]), shared by the node and the edge classifier: upload() reserves
// the caller's buffers and copies its inputs (behind the reservations made here: every allocation of a call comes before its
// first copy), enqueue(loss_dev) puts one loss-and-gradient of theta on ctx->stream (f.grad; the loss also to *loss_dev).
// The beta powers are float64 products.  Reads back theta, the loss of every iteration and the device time of the loop.
template <class Upload, class Enqueue>
int adam_fit(gg_ctx *ctx, const char *fn, AdamBufs &f, size_t n_w, size_t n_b, int iters, float lr, Upload upload, Enqueue enqueue, float *W_inout,
             float *b_inout, float *loss_out, double *ms_out) {
    const size_t n_par = n_w + n_b;
    GG_HIP_FN(f.mom.reserve(sizeof(float) * n_par));
    GG_HIP_FN(f.var.reserve(sizeof(float) * n_par));
    GG_HIP_FN(f.loss.reserve(sizeof(float) * iters));
    GG_HIP_FN(upload());
    GG_HIP_FN(hipMemsetAsync(f.mom.p, 0, sizeof(float) * n_par, ctx->stream));
    GG_HIP_FN(hipMemsetAsync(f.var.p, 0, sizeof(float) * n_par, ctx->stream));
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    double b1p = 1.0, b2p = 1.0;
    for (int t = 0; t < iters; ++t) {
        b1p *= 0.9;
        b2p *= 0.999;
        enqueue(f.loss.as<float>() + t);
        hipLaunchKernelGGL(nc_adam_kernel, dim3(cdiv(n_par, 256)), dim3(256), 0, ctx->stream, f.theta.as<float>(), f.mom.as<float>(), f.var.as<float>(),
                           f.grad.as<float>(), (int64_t)n_par, lr, (float)(1.0 - b1p), (float)(1.0 - b2p));
    }
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    GG_HIP_FN(hipGetLastError());
    GG_HIP_FN(hipMemcpyAsync(W_inout, f.theta.p, sizeof(float) * n_w, hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipMemcpyAsync(b_inout, f.theta.as<float>() + n_w, sizeof(float) * n_b, hipMemcpyDeviceToHost, ctx->stream));
    if (loss_out) GG_HIP_FN(hipMemcpyAsync(loss_out, f.loss.p, sizeof(float) * iters, hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    if (ms_out) *ms_out = ms;
    return GG_OK;
}

// gg_classifier_fit / gg_classifier_ml_fit
int fit_call(gg_ctx *ctx, const char *fn, bool ml, int which, const int32_t *nodes, const void *labels, int64_t m, int n_class, int iters, float lr,
             float l2, float *W_inout, float *b_inout, float *loss_out, double *ms_out) {
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (const int rc = check_common(ctx, fn, which, nodes, m, n_class)) return rc;
    if (const int rc = check_any_labels(ctx, fn, ml, labels, m, n_class)) return rc;
    GG_CHECK(ctx, W_inout && b_inout, GG_EINVAL, "%s: W_inout and b_inout must not be NULL", fn);
    GG_CHECK(ctx, iters >= 1 && iters <= 1000000, GG_EINVAL, "%s: iters = %d outside [1, 1000000]", fn, iters);
    GG_CHECK(ctx, lr > 0.f && std::isfinite(lr), GG_EINVAL, "%s: lr must be finite and > 0", fn);
    GG_CHECK(ctx, l2 >= 0.f && std::isfinite(l2), GG_EINVAL, "%s: l2 must be finite and >= 0", fn);
    GG_HIP(ctx, hipSetDevice(ctx->device));
    const int C = n_class;
    const size_t cd = (size_t)C * ctx->n_emb;
    const SweepPlan p = sweep_plan(m, C, ctx->ld, ml);
    Fit f;
    return adam_fit(
        ctx, fn, f, cd, C, iters, lr, [&] { return fit_upload(ctx, f, p, ml, nodes, labels, m, C, W_inout, b_inout); },
        [&](float *loss_dev) { enqueue_lossgrad(ctx, f, p, which, m, C, l2, loss_dev); }, W_inout, b_inout, loss_out, ms_out);
}

// gg_classifier_predict / gg_classifier_ml_predict: `pred_out` is int32 [m] (the argmax), or with `ml` the mask words uint32
// [m][ceil(C / 32)] of the first k[i] classes (k given) or of the classes with a positive logit (k NULL; `k` is the ml form's alone)
int predict_call(gg_ctx *ctx, const char *fn, bool ml, int which, const int32_t *nodes, int64_t m, int n_class, const float *W, const float *b,
                 const int32_t *k, void *pred_out, float *logits_out) {
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (const int rc = check_common(ctx, fn, which, nodes, m, n_class)) return rc;
    GG_CHECK(ctx, W && b && pred_out, GG_EINVAL, "%s: W, b and %s must not be NULL", fn, ml ? "pred_bits" : "pred_out");
    if (k)
        for (int64_t i = 0; i < m; ++i)
            GG_CHECK(ctx, k[i] >= 0 && k[i] <= n_class, GG_EINVAL, "%s: k = %d (row %lld) outside [0, n_class = %d]", fn, k[i], (long long)i, n_class);
    GG_HIP(ctx, hipSetDevice(ctx->device));
    const int C = n_class, d = ctx->n_emb, ld = ctx->ld;
    const size_t cd = (size_t)C * d, pred_bytes = sizeof(int32_t) * (size_t)m * (ml ? cdiv(C, 32) : 1), logit_bytes = sizeof(float) * (size_t)m * C;
    // W [C][ld + 1], a row per wavefront, and the ml form's published logits per wavefront
    const size_t lds = sizeof(float) * ((size_t)C * (ld + 1) + 4 * (size_t)ld + (ml ? 4 * (size_t)RT_MAX_OUT : 0));
    const void *kernel = ml ? (const void *)nc_ml_predict_kernel : (const void *)nc_predict_kernel;
    ScopedBuf d_nodes, d_theta, d_k, d_pred, d_logits;
    GG_HIP_FN(d_nodes.reserve(sizeof(int32_t) * m));
    GG_HIP_FN(d_theta.reserve(sizeof(float) * (cd + C)));
    if (k) GG_HIP_FN(d_k.reserve(sizeof(int32_t) * m));
    GG_HIP_FN(d_pred.reserve(pred_bytes));
    if (logits_out) GG_HIP_FN(d_logits.reserve(logit_bytes));
    GG_HIP_FN(upload_nodes_theta(ctx, d_nodes, d_theta, nodes, m, C, W, b));
    if (k) GG_HIP_FN(hipMemcpyAsync(d_k.p, k, sizeof(int32_t) * m, hipMemcpyHostToDevice, ctx->stream));
    if (lds > 48 * 1024) GG_HIP_FN(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const dim3 grid((unsigned)std::min<int64_t>(1024, (m + 3) / 4));
    const float *E = ctx->model[which].E, *dW = d_theta.as<float>(), *db = dW + cd;
    if (ml) {
        hipLaunchKernelGGL(nc_ml_predict_kernel, grid, dim3(256), lds, ctx->stream, E, ld, d, d_nodes.as<int32_t>(), m, C, dW, db, d_k.as<int32_t>(),
                           d_pred.as<uint32_t>(), d_logits.as<float>());
    } else {
        hipLaunchKernelGGL(nc_predict_kernel, grid, dim3(256), lds, ctx->stream, E, ld, d, d_nodes.as<int32_t>(), m, C, dW, db, d_pred.as<int32_t>(),
                           d_logits.as<float>());
    }
    GG_HIP_FN(hipGetLastError());
    GG_HIP_FN(hipMemcpyAsync(pred_out, d_pred.p, pred_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (logits_out) GG_HIP_FN(hipMemcpyAsync(logits_out, d_logits.p, logit_bytes, hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipStreamSynchronize(ctx->stream));
    return GG_OK;
}

// ---- gg_edge_classifier_*: the host side
struct EdgePlan {
    int grid, NJ;
};

EdgePlan edge_plan(int64_t m, int ld, int max_grid) {
    return EdgePlan{(int)std::min<int64_t>(max_grid, (m + EC_EDGES - 1) / EC_EDGES), cdiv(ld, 4 * EC_LANES)};
}

// device state of an edge fit or loss-and-gradient call; theta = (w [d], b [1])
struct EdgeFit : AdamBufs {
    ScopedBuf u, v, y, part;
};

int check_edges(gg_ctx *ctx, const char *fn, int which, int op, const int32_t *u, const int32_t *v, int64_t m) {
    GG_CHECK(ctx, which == 0 || which == 1, GG_EINVAL, "%s: which must be 0 (generator) or 1 (discriminator), got %d", fn, which);
    GG_CHECK(ctx, op >= 0 && op <= 3, GG_EINVAL, "%s: op = %d outside [0, 3] (0 Hadamard, 1 average, 2 L1, 3 L2)", fn, op);
    GG_CHECK(ctx, m >= 1 && m <= 0x7fffffffLL, GG_EINVAL, "%s: m = %lld outside [1, 2^31 - 1]", fn, (long long)m);
    GG_CHECK(ctx, ctx->n_emb <= RT_MAX_D, GG_EINVAL, "%s: supports n_emb <= %d (got %d)", fn, RT_MAX_D, ctx->n_emb);
    GG_CHECK(ctx, u != nullptr, GG_EINVAL, "%s: u is NULL", fn);
    GG_CHECK(ctx, v != nullptr, GG_EINVAL, "%s: v is NULL", fn);
    for (int64_t i = 0; i < m; ++i) {
        GG_CHECK(ctx, u[i] >= 0 && u[i] < ctx->n_node, GG_EINVAL, "%s: node id u = %d (entry %lld) outside [0, %d)", fn, u[i], (long long)i, ctx->n_node);
        GG_CHECK(ctx, v[i] >= 0 && v[i] < ctx->n_node, GG_EINVAL, "%s: node id v = %d (entry %lld) outside [0, %d)", fn, v[i], (long long)i, ctx->n_node);
    }
    return GG_OK;
}

int check_edge_labels(gg_ctx *ctx, const char *fn, const int32_t *y, int64_t m) {
    GG_CHECK(ctx, y != nullptr, GG_EINVAL, "%s: y is NULL", fn);
    for (int64_t i = 0; i < m; ++i) GG_CHECK(ctx, y[i] == 0 || y[i] == 1, GG_EINVAL, "%s: y = %d (entry %lld) is neither 0 nor 1", fn, y[i], (long long)i);
    return GG_OK;
}

// the edges, the labels (y may be NULL: prediction) and theta = (w, b) on the device; every allocation comes before the first copy
hipError_t edge_upload(gg_ctx *ctx, EdgeFit &f, const int32_t *u, const int32_t *v, const int32_t *y, int64_t m, const float *w, const float *b) {
    const size_t d = ctx->n_emb, ids = sizeof(int32_t) * (size_t)m;
    hipError_t e = f.u.reserve(ids);
    if (e == hipSuccess) e = f.v.reserve(ids);
    if (e == hipSuccess && y) e = f.y.reserve(ids);
    if (e == hipSuccess) e = f.theta.reserve(sizeof(float) * (d + 1));
    if (e == hipSuccess) e = hipMemcpyAsync(f.u.p, u, ids, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(f.v.p, v, ids, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && y) e = hipMemcpyAsync(f.y.p, y, ids, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(f.theta.p, w, sizeof(float) * d, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(f.theta.as<float>() + d, b, sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    return e;
}

// edge sweep + reduce of theta on ctx->stream: grad [d + 2] = gw, gb, loss; the loss also to *loss_dev
void enqueue_edge_lossgrad(gg_ctx *ctx, const EdgeFit &f, const EdgePlan &p, int which, int op, int64_t m, float l2, float *loss_dev) {
    const int d = ctx->n_emb;
    EdgeArgs a{ctx->model[which].E, f.u.as<int32_t>(), f.v.as<int32_t>(), f.y.as<int32_t>(), m, ctx->ld, d, f.theta.as<float>(), f.theta.as<float>() + d,
               f.part.as<float>(), nullptr};
    hipLaunchKernelGGL(ec_sweeps[op][p.NJ - 1], dim3(p.grid), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(nc_reduce_kernel, dim3(cdiv(d + 1, NC_RED_COLS) + 1), dim3(256), 0, ctx->stream, f.part.as<float>(), p.grid, 1, d, m,
                       f.theta.as<float>(), l2, f.grad.as<float>(), loss_dev);
}

int edge_lossgrad_call(gg_ctx *ctx, int which, int op, const int32_t *u, const int32_t *v, const int32_t *y, int64_t m, const float *w, const float *b,
                       float l2, float *loss_out, float *gw_out, float *gb_out) {
    const char *fn = "gg_edge_classifier_lossgrad";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (const int rc = check_edges(ctx, fn, which, op, u, v, m)) return rc;
    if (const int rc = check_edge_labels(ctx, fn, y, m)) return rc;
    GG_CHECK(ctx, w && b && loss_out && gw_out && gb_out, GG_EINVAL, "%s: w, b, loss_out, gw_out, gb_out must not be NULL", fn);
    GG_CHECK(ctx, l2 >= 0.f && std::isfinite(l2), GG_EINVAL, "%s: l2 must be finite and >= 0", fn);
    GG_HIP(ctx, hipSetDevice(ctx->device));
    const size_t d = ctx->n_emb;
    const EdgePlan p = edge_plan(m, ctx->ld, EC_MAX_GRID);
    EdgeFit f;
    GG_HIP_FN(f.grad.reserve(sizeof(float) * (d + 2)));
    GG_HIP_FN(f.part.reserve(sizeof(float) * (d + 3) * p.grid));
    GG_HIP_FN(edge_upload(ctx, f, u, v, y, m, w, b));
    enqueue_edge_lossgrad(ctx, f, p, which, op, m, l2, nullptr);
    GG_HIP_FN(hipGetLastError());
    GG_HIP_FN(hipMemcpyAsync(gw_out, f.grad.p, sizeof(float) * d, hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipMemcpyAsync(gb_out, f.grad.as<float>() + d, sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipMemcpyAsync(loss_out, f.grad.as<float>() + d + 1, sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipStreamSynchronize(ctx->stream));
    return GG_OK;
}

int edge_fit_call(gg_ctx *ctx, int which, int op, const int32_t *u, const int32_t *v, const int32_t *y, int64_t m, int iters, float lr, float l2,
                  float *w_inout, float *b_inout, float *loss_out, double *ms_out) {
    const char *fn = "gg_edge_classifier_fit";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (const int rc = check_edges(ctx, fn, which, op, u, v, m)) return rc;
    if (const int rc = check_edge_labels(ctx, fn, y, m)) return rc;
    GG_CHECK(ctx, w_inout && b_inout, GG_EINVAL, "%s: w_inout and b_inout must not be NULL", fn);
    GG_CHECK(ctx, iters >= 1 && iters <= 1000000, GG_EINVAL, "%s: iters = %d outside [1, 1000000]", fn, iters);
    GG_CHECK(ctx, lr > 0.f && std::isfinite(lr), GG_EINVAL, "%s: lr must be finite and > 0", fn);
    GG_CHECK(ctx, l2 >= 0.f && std::isfinite(l2), GG_EINVAL, "%s: l2 must be finite and >= 0", fn);
    GG_HIP(ctx, hipSetDevice(ctx->device));
    const size_t d = ctx->n_emb;
    const EdgePlan p = edge_plan(m, ctx->ld, EC_MAX_GRID);
    EdgeFit f;
    auto upload = [&] {
        hipError_t e = f.grad.reserve(sizeof(float) * (d + 2));
        if (e == hipSuccess) e = f.part.reserve(sizeof(float) * (d + 3) * p.grid);
        if (e == hipSuccess) e = edge_upload(ctx, f, u, v, y, m, w_inout, b_inout);
        return e;
    };
    return adam_fit(
        ctx, fn, f, d, 1, iters, lr, upload, [&](float *loss_dev) { enqueue_edge_lossgrad(ctx, f, p, which, op, m, l2, loss_dev); }, w_inout, b_inout,
        loss_out, ms_out);
}

int edge_predict_call(gg_ctx *ctx, int which, int op, const int32_t *u, const int32_t *v, int64_t m, const float *w, const float *b, float *logits_out) {
    const char *fn = "gg_edge_classifier_predict";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (const int rc = check_edges(ctx, fn, which, op, u, v, m)) return rc;
    GG_CHECK(ctx, w && b && logits_out, GG_EINVAL, "%s: w, b and logits_out must not be NULL", fn);
    GG_HIP(ctx, hipSetDevice(ctx->device));
    const int d = ctx->n_emb;
    const EdgePlan p = edge_plan(m, ctx->ld, EC_PREDICT_GRID);
    EdgeFit f;
    ScopedBuf d_logits;
    GG_HIP_FN(d_logits.reserve(sizeof(float) * (size_t)m));
    GG_HIP_FN(edge_upload(ctx, f, u, v, nullptr, m, w, b));
    EdgeArgs a{ctx->model[which].E, f.u.as<int32_t>(), f.v.as<int32_t>(), nullptr, m, ctx->ld, d, f.theta.as<float>(), f.theta.as<float>() + d, nullptr,
               d_logits.as<float>()};
    hipLaunchKernelGGL(ec_predicts[op][p.NJ - 1], dim3(p.grid), dim3(256), 0, ctx->stream, a);
    GG_HIP_FN(hipGetLastError());
    GG_HIP_FN(hipMemcpyAsync(logits_out, d_logits.p, sizeof(float) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipStreamSynchronize(ctx->stream));
    return GG_OK;
}

}  // namespace

}  // namespace gg

using namespace gg;

// gg_classifier_lossgrad, gg_classifier_fit and their multi-label forms: see include/graphgan_hip.h.
extern "C" int gg_classifier_lossgrad(gg_ctx *ctx, int which, const int32_t *nodes, const int32_t *labels, int64_t m, int n_class, const float *W,
                                      const float *b, float l2, float *loss_out, float *gW_out, float *gb_out) {
    return lossgrad_call(ctx, "gg_classifier_lossgrad", false, which, nodes, labels, m, n_class, W, b, l2, loss_out, gW_out, gb_out);
}

extern "C" int gg_classifier_ml_lossgrad(gg_ctx *ctx, int which, const int32_t *nodes, const uint32_t *label_bits, int64_t m, int n_class,
                                         const float *W, const float *b, float l2, float *loss_out, float *gW_out, float *gb_out) {
    return lossgrad_call(ctx, "gg_classifier_ml_lossgrad", true, which, nodes, label_bits, m, n_class, W, b, l2, loss_out, gW_out, gb_out);
}

extern "C" int gg_classifier_fit(gg_ctx *ctx, int which, const int32_t *nodes, const int32_t *labels, int64_t m, int n_class, int iters, float lr,
                                 float l2, float *W_inout, float *b_inout, float *loss_out, double *ms_out) {
    return fit_call(ctx, "gg_classifier_fit", false, which, nodes, labels, m, n_class, iters, lr, l2, W_inout, b_inout, loss_out, ms_out);
}

extern "C" int gg_classifier_ml_fit(gg_ctx *ctx, int which, const int32_t *nodes, const uint32_t *label_bits, int64_t m, int n_class, int iters,
                                    float lr, float l2, float *W_inout, float *b_inout, float *loss_out, double *ms_out) {
    return fit_call(ctx, "gg_classifier_ml_fit", true, which, nodes, label_bits, m, n_class, iters, lr, l2, W_inout, b_inout, loss_out, ms_out);
}

// gg_classifier_predict, gg_classifier_ml_predict: see include/graphgan_hip.h.
extern "C" int gg_classifier_predict(gg_ctx *ctx, int which, const int32_t *nodes, int64_t m, int n_class, const float *W, const float *b,
                                     int32_t *pred_out, float *logits_out) {
    return predict_call(ctx, "gg_classifier_predict", false, which, nodes, m, n_class, W, b, nullptr, pred_out, logits_out);
}

extern "C" int gg_classifier_ml_predict(gg_ctx *ctx, int which, const int32_t *nodes, int64_t m, int n_class, const float *W, const float *b,
                                        const int32_t *k, uint32_t *pred_bits, float *logits_out) {
    return predict_call(ctx, "gg_classifier_ml_predict", true, which, nodes, m, n_class, W, b, k, pred_bits, logits_out);
}

// gg_edge_classifier_lossgrad, gg_edge_classifier_fit, gg_edge_classifier_predict: see include/graphgan_hip.h.
extern "C" int gg_edge_classifier_lossgrad(gg_ctx *ctx, int which, int op, const int32_t *u, const int32_t *v, const int32_t *y, int64_t m,
                                           const float *w, const float *b, float l2, float *loss_out, float *gw_out, float *gb_out) {
    return edge_lossgrad_call(ctx, which, op, u, v, y, m, w, b, l2, loss_out, gw_out, gb_out);
}

extern "C" int gg_edge_classifier_fit(gg_ctx *ctx, int which, int op, const int32_t *u, const int32_t *v, const int32_t *y, int64_t m, int iters,
                                      float lr, float l2, float *w_inout, float *b_inout, float *loss_out, double *ms_out) {
    return edge_fit_call(ctx, which, op, u, v, y, m, iters, lr, l2, w_inout, b_inout, loss_out, ms_out);
}

extern "C" int gg_edge_classifier_predict(gg_ctx *ctx, int which, int op, const int32_t *u, const int32_t *v, int64_t m, const float *w,
                                          const float *b, float *logits_out) {
    return edge_predict_call(ctx, which, op, u, v, m, w, b, logits_out);
}
