// gram.hip -- the centred Gram matrix of M gathered rows of a resident table: the device part of the PCA of the embedding rows.
//     c_i = x_i - center (ONE fp32 subtraction per entry; no centre: c_i = x_i),   x_i = E[nodes[i]]
//     G = sum_i c_i c_i^T  [d, d],   s = sum_i c_i  [d]
// gram_sweep_kernel<DT, GRAM> is the hot path.  A persistent workgroup (256 threads, 4 wavefronts) walks 64-row tiles, round
// robin over the grid = min(GRAM_MAX_GRID, ceil(M / 64)) -- the rule of row_tiles.h, a function of M alone.  Per tile
//   1. the rows are gathered as float4 into LDS Xs[64][32 DT + 1] (the odd stride of RowTiles), the centre subtracted on the way
//      in; the next tile's rows are already in flight to registers while this one computes, and the node ids of the tile after
//      that are in flight beside them (a row fetch never waits for its id).  Rows behind M are ZEROS (not
//      0 - center), columns behind d are zeros of the table's padding minus a zero of the staged centre;
//   2. thread j < 32 DT continues the fp32 chain s_j = s_j + Xs[r][j], r ascending: the workgroup's column sums;
//   3. with GRAM the product Xs^T . Xs on v_mfma_f32_32x32x2_f32, BOTH operands read from the tile: only the T = DT (DT + 1) / 2
//      output tiles (a, b), a <= b, of the 32 x 32 tiling are computed (the result is symmetric), tile t = wv + 4 i by wavefront
//      wv, its accumulators in registers across all tiles of the workgroup (9 tiles = 144 registers per lane at d = 256).  k runs
//      over the 64 rows ascending, so part[j][l] is bit for bit the k-ordered fmaf chain from 0.0 of c_ij c_il over the
//      workgroup's rows in ascending order.  The LDS reads of 8 k-steps of TWO output tiles are issued ahead of their 16 matrix
//      instructions, which alternate between the two accumulators (independent chains: the instruction's dependent-accumulator
//      latency is hidden behind the other tile's).
// GRAM = false is the mean pass: gather, subtract, column sums; it pays for no product.
// Every workgroup writes its partial to a stage (part [grid][d][d], upper tiles only; psum [grid][d]) and gram_reduce_kernel adds
// the stage in float64, workgroups ascending, one thread per entry; an entry below the tile diagonal is the COPY of its mirror.
// No floating-point atomics: the same inputs and table give the same bits.
#include <math.h>

#include <algorithm>

#include "row_tiles.h"

namespace gg {

namespace {

constexpr int GRAM_MAX_GRID = 512;  // workgroups of a sweep, at most: the stage is grid x d x d floats (134 MB at d = 256)

struct GramArgs {
    const float *E;          // [n_node, ld]
    const int32_t *nodes;
    int64_t m;
    int ld, d;
    const float *center;     // [d] on the device, or NULL
    float *part;             // [grid][d][d] (GRAM)
    float *psum;             // [grid][d]
};

// output tile t of the upper triangle, row-major: (0, 0) .. (0, DT - 1), (1, 1) ..
template <int DT>
__device__ __forceinline__ void gram_tile(int t, int &a, int &b) {
    a = 0;
    int len = DT;
#pragma unroll
    for (int q = 0; q < DT - 1; ++q)
        if (t >= len) {
            t -= len;
            --len;
            ++a;
        }
    b = a + t;
}

template <int DT, bool GRAM>
__global__ __launch_bounds__(256) void gram_sweep_kernel(GramArgs g) {
    constexpr int XS = 32 * DT + 1, NPF = 2 * DT, T = DT * (DT + 1) / 2, NT = GRAM ? (T + 3) / 4 : 1;
    extern __shared__ float gram_lds[];  // Xs [64][XS]
    __shared__ float4 cs4[64];           // the centre, columns behind d: zeros
    __shared__ int32_t ids[RT_ROWS];     // node ids of the tile whose rows are fetched next
    float *Xs = gram_lds;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int ld = g.ld, d = g.d;
    const int64_t m = g.m, n_tiles = (m + RT_ROWS - 1) / RT_ROWS;

    // The node ids run one tile ahead of the rows: thread r < 64 loads the id of row r of the tile after next into a register
    // while this tile computes and leaves it in ids[] behind the products, so a row fetch never waits for its id first.
    // -1: a row behind M.
    int32_t next_id = -1;
    auto fetch_id = [&](int64_t tile) {
        const int64_t row = tile * RT_ROWS + tid;
        next_id = (tid < RT_ROWS && tile < n_tiles && row < m) ? g.nodes[row] : -1;
    };
    float4 pf[NPF];
    auto fetch = [&]() {  // the rows of ids[] -> registers (rows behind M and columns behind ld: zeros)
#pragma unroll
        for (int j = 0; j < NPF; ++j) {
            const int i = tid + 256 * j, r = i / (8 * DT), col = (i % (8 * DT)) * 4;
            const int32_t id = ids[r];
            pf[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (id >= 0 && col < ld) pf[j] = *(const float4 *)(g.E + (int64_t)id * ld + col);
        }
    };

    fetch_id(blockIdx.x);
    if (tid < RT_ROWS) ids[tid] = next_id;
    ((float *)cs4)[tid] = (g.center && tid < d) ? g.center[tid] : 0.f;
    fetch_id((int64_t)blockIdx.x + gridDim.x);
    __syncthreads();
    fetch();
    __syncthreads();  // (ids[] has been read)
    if (tid < RT_ROWS) ids[tid] = next_id;

    // this wavefront's output tiles: LDS column offsets of the two operands
    int ca[NT], cb[NT];
    f32x16 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        int a = 0, b = 0;
        gram_tile<DT>(min(wv + 4 * i, T - 1), a, b);
        ca[i] = 32 * a + l31;
        cb[i] = 32 * b + l31;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[i][q] = 0.f;
    }
    float colsum = 0.f;

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = tile * RT_ROWS;
        __syncthreads();  // the previous tile's sums and products have read Xs, ids[] holds the next tile's (first tile: the centre is staged)
#pragma unroll
        for (int j = 0; j < NPF; ++j) {
            const int i = tid + 256 * j, r = i / (8 * DT), col = (i % (8 * DT)) * 4;
            const bool valid = row0 + r < m;
            const float4 c = cs4[col >> 2];
            float *x = Xs + r * XS + col;
            x[0] = valid ? pf[j].x - c.x : 0.f;
            x[1] = valid ? pf[j].y - c.y : 0.f;
            x[2] = valid ? pf[j].z - c.z : 0.f;
            x[3] = valid ? pf[j].w - c.w : 0.f;
        }
        fetch();
        fetch_id(tile + 2 * (int64_t)gridDim.x);
        __syncthreads();

        // column sums: thread j owns column j (odd row stride: conflict-free), 8 loads issued together, the adds in row order
        if (tid < 32 * DT) {
            const float *x = Xs + tid;
#pragma unroll
            for (int r0 = 0; r0 < RT_ROWS; r0 += 8) {
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = x[(r0 + e) * XS];
#pragma unroll
                for (int e = 0; e < 8; ++e) colsum = colsum + v[e];
            }
        }

        if constexpr (GRAM) {
            // k over the 64 rows in 4 batches of 8 steps; per batch the wavefront's tiles two at a time
#pragma unroll 1
            for (int kb = 0; kb < RT_ROWS; kb += 16) {
                const float *xk = Xs + (kb + half) * XS;
#pragma unroll
                for (int i = 0; i < NT; i += 2) {
                    if (i + 1 < NT && wv + 4 * (i + 1) < T) {
                        float a0[8], b0[8], a1[8], b1[8];
#pragma unroll
                        for (int s = 0; s < 8; ++s) {
                            a0[s] = xk[2 * s * XS + ca[i]];
                            b0[s] = xk[2 * s * XS + cb[i]];
                            a1[s] = xk[2 * s * XS + ca[i + 1 < NT ? i + 1 : i]];
                            b1[s] = xk[2 * s * XS + cb[i + 1 < NT ? i + 1 : i]];
                        }
#pragma unroll
                        for (int s = 0; s < 8; ++s) {
                            acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b0[s], acc[i], 0, 0, 0);
                            acc[i + 1 < NT ? i + 1 : i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b1[s], acc[i + 1 < NT ? i + 1 : i], 0, 0, 0);
                        }
                    } else if (wv + 4 * i < T) {
                        float a0[8], b0[8];
#pragma unroll
                        for (int s = 0; s < 8; ++s) {
                            a0[s] = xk[2 * s * XS + ca[i]];
                            b0[s] = xk[2 * s * XS + cb[i]];
                        }
#pragma unroll
                        for (int s = 0; s < 8; ++s) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b0[s], acc[i], 0, 0, 0);
                    }
                }
            }
        }
        if (tid < RT_ROWS) ids[tid] = next_id;  // (every fetch of this tile read ids[] in front of the barrier above)
    }

    if (tid < d) g.psum[(int64_t)blockIdx.x * d + tid] = colsum;
    if constexpr (GRAM) {
        float *part = g.part + (int64_t)blockIdx.x * d * d;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            if (wv + 4 * i < T) {
                const int col = cb[i];
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int c = ca[i] - l31 + tile_row(reg, half);
                    if (c < d && col < d) part[(int64_t)c * d + col] = acc[i][reg];
                }
            }
        }
    }
}

// The totals of a sweep from its stage: float64, workgroups ascending, one thread per entry.  Entries [0, d) are the sums; with
// with_gram entries d + j d + l are gram[j][l] for tile(j) <= tile(l), and the thread writes the mirror entry gram[l][j] too
// where the tiles differ (inside a diagonal tile both entries were computed, by the same chain: equal bits).
__global__ __launch_bounds__(256) void gram_reduce_kernel(const float *part, const float *psum, int n_part, int d, int with_gram, double *sums, double *gram) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, dd = (int64_t)d * d;
    if (idx >= d + (with_gram ? dd : 0)) return;
    const float *src;
    int64_t stride;
    int j = 0, l = 0;
    if (idx < d) {
        src = psum + idx;
        stride = d;
    } else {
        j = (int)((idx - d) / d);
        l = (int)((idx - d) - (int64_t)j * d);
        if ((j >> 5) > (l >> 5)) return;
        src = part + (int64_t)j * d + l;
        stride = dd;
    }
    double s = 0.0;
    int w = 0;
    for (; w + 8 <= n_part; w += 8) {  // (the 8 loads are issued together; the adds stay in order)
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = src[(int64_t)(w + e) * stride];
#pragma unroll
        for (int e = 0; e < 8; ++e) s += (double)v[e];
    }
    for (; w < n_part; ++w) s += (double)src[(int64_t)w * stride];
    if (idx < d) {
        sums[idx] = s;
    } else {
        gram[(int64_t)j * d + l] = s;
        if ((j >> 5) < (l >> 5)) gram[(int64_t)l * d + j] = s;
    }
}

typedef void (*GramFn)(GramArgs);
#define GRAM_ROW(s) {gram_sweep_kernel<1, s>, gram_sweep_kernel<2, s>, gram_sweep_kernel<3, s>, gram_sweep_kernel<4, s>, \
                     gram_sweep_kernel<5, s>, gram_sweep_kernel<6, s>, gram_sweep_kernel<7, s>, gram_sweep_kernel<8, s>}
// [0]: sums only, [1]: with the products
const GramFn gram_sweeps[2][8] = {GRAM_ROW(false), GRAM_ROW(true)};

int gram_call(gg_ctx *ctx, int which, const int32_t *nodes, int64_t m, const float *center, double *sums_out, double *gram_out, double *ms_out) {
    const char *fn = "gg_gram";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (const int rc = check_rows(ctx, fn, which, nodes, m, [] { return (int)GG_OK; })) return rc;
    const int d = ctx->n_emb, ld = ctx->ld;
    if (center)
        for (int j = 0; j < d; ++j) GG_CHECK(ctx, std::isfinite(center[j]), GG_EINVAL, "%s: center[%d] = %g is not finite", fn, j, (double)center[j]);
    GG_HIP(ctx, hipSetDevice(ctx->device));
    const bool with_gram = gram_out != nullptr;
    const int DT = cdiv(ld, 32), grid = (int)std::min<int64_t>(GRAM_MAX_GRID, (m + RT_ROWS - 1) / RT_ROWS);
    const size_t lds = sizeof(float) * RT_ROWS * (32 * DT + 1), dd = (size_t)d * d;
    const GramFn kern = gram_sweeps[with_gram ? 1 : 0][DT - 1];
    ScopedBuf b_nodes, b_center, b_part, b_psum, b_sums, b_gram;
    hipError_t e = b_nodes.reserve(sizeof(int32_t) * m);
    if (e == hipSuccess && center) e = b_center.reserve(sizeof(float) * d);
    if (e == hipSuccess && with_gram) e = b_part.reserve(sizeof(float) * dd * grid);
    if (e == hipSuccess) e = b_psum.reserve(sizeof(float) * (size_t)d * grid);
    if (e == hipSuccess) e = b_sums.reserve(sizeof(double) * d);
    if (e == hipSuccess && with_gram) e = b_gram.reserve(sizeof(double) * dd);
    if (e == hipSuccess) e = hipMemcpyAsync(b_nodes.p, nodes, sizeof(int32_t) * m, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && center) e = hipMemcpyAsync(b_center.p, center, sizeof(float) * d, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && lds > 48 * 1024) e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    GG_HIP_FN(e);
    GramArgs a{ctx->model[which].E, b_nodes.as<int32_t>(), m, ld, d, b_center.as<float>(), b_part.as<float>(), b_psum.as<float>()};
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, ctx->stream, a);
    hipLaunchKernelGGL(gram_reduce_kernel, dim3(cdiv((int64_t)d + (with_gram ? dd : 0), 256)), dim3(256), 0, ctx->stream, b_part.as<float>(),
                       b_psum.as<float>(), grid, d, with_gram ? 1 : 0, b_sums.as<double>(), b_gram.as<double>());
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    GG_HIP_FN(hipGetLastError());
    if (sums_out) GG_HIP_FN(hipMemcpyAsync(sums_out, b_sums.p, sizeof(double) * d, hipMemcpyDeviceToHost, ctx->stream));
    if (gram_out) GG_HIP_FN(hipMemcpyAsync(gram_out, b_gram.p, sizeof(double) * dd, hipMemcpyDeviceToHost, ctx->stream));
    GG_HIP_FN(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    if (ms_out) *ms_out = ms;
    return GG_OK;
}

}  // namespace

}  // namespace gg

using namespace gg;

// gg_gram: see include/graphgan_hip.h.
extern "C" int gg_gram(gg_ctx *ctx, int which, const int32_t *nodes, int64_t m, const float *center, double *sums_out, double *gram_out, double *ms_out) {
    return gram_call(ctx, which, nodes, m, center, sums_out, gram_out, ms_out);
}
