// row_tiles.h -- the matrix-core sweep over M gathered rows of a resident table, written once for its two users: the classifier
// (classifier.hip, nc_sweep_kernel: logits, loss stage, gradient) and k-means (kmeans.hip, km_sweep_kernel: distances, argmin,
// cluster sums).  A persistent workgroup (256 threads, 4 wavefronts) walks 64-row tiles, round robin over the grid; per tile
//   1. the rows are gathered into LDS (Xs; the next tile's rows are already in flight to registers while this one computes),
//   2. FIRST PRODUCT  P[64, n_out] = Xs . W^T on v_mfma_f32_32x32x2_f32, the second operand W [n_out, d] (class weights, centroids)
//      staged in LDS (Ws) once per workgroup -- in k-chunks per tile only where n_out x d does not fit beside the tile: n_out > 96
//      at ld > 152 and n_out > 64 at ld > 192 (row_tile_plan; six of the 32 (CT, DT) instances at full tiles: (4, 5 .. 8), (3, 7),
//      (3, 8)); the accumulators are scattered to LDS (Ps),
//   3. the user's ROW STAGE rows(row0, Xs, Ps): row tid >> 2 of the tile by 4 threads (strides RowTiles<CT, DT>::XS, ::PS); it
//      reads P and leaves the factor of the second product in its place (rows behind M and columns behind n_out: zeros),
//   4. with SECOND: column(Ps[r][tid]) for r ascending, thread tid < n_out owning a column, and the SECOND PRODUCT
//      G[n_out, d] += Ps^T . Xs on the same matrix instruction, its accumulators in registers across all tiles of the workgroup.
// CT = ceil(n_out / 32) and DT = ceil(ld / 32) are template parameters: the accumulators are register arrays with compile-time
// indices, and every function here is __forceinline__ (an instantiation that spills, or a stage behind a call, fails the build:
// check_no_scratch.sh).  Both products run kk ascending: bit for bit k-ordered fmaf chains from 0.0.
// Determinism: the grid is min(RT_MAX_GRID, ceil(M / 64)) -- a function of M alone --, every workgroup writes a partial to a stage
// that the user's reducer adds in a fixed order; no floating-point atomics.  A float64 sum of a workgroup leaves as two floats
// (high part, remainder): one float would round a sum of 64-row terms at 2^-24 of ITS size, more than half a float32 spacing of
// the mean at small M.
// Behind the device part: the launch plan and the host helpers both files share.
#pragma once
#include <algorithm>

#include "score_tiles.h"

namespace gg {

constexpr int RT_ROWS = 64;         // rows per tile
constexpr int RT_MAX_GRID = 512;    // workgroups of a sweep, at most
constexpr int RT_MAX_OUT = 128, RT_MAX_D = 256;  // n_out (classes, clusters) and d, at most
constexpr size_t RT_LDS = 150 * 1024;  // dynamic LDS of a sweep workgroup, at most

// compile-time geometry of an instance
template <int CT, int DT, bool SECOND = true>
struct RowTiles {
    static constexpr int XS = 32 * DT + 1, PS = 32 * CT + 1;       // row strides of Xs / Ps (odd: conflict-free column walks)
    static constexpr int N1 = (2 * CT + 3) / 4;                     // first-product tiles (row half, output tile) per wavefront
    static constexpr int N2 = SECOND ? (CT * DT + 3) / 4 : 1;       // second-product tiles (output tile, column tile) per wavefront
    static constexpr int NPF = 2 * DT;                              // float4 pieces of a tile per thread
};

// The sweep of a workgroup over its tiles.  lds: the dynamic LDS, carved up as Xs [64][XS] | Ps [64][PS] | Ws [32 CT][KW + 1];
// KW: the k-chunk of the W staging (>= ld: W is staged once, before setup).  setup(Ws, WS, resident) runs once behind the first
// tile's gather and the resident staging (no barrier in between: a setup that reads Ws brings its own).  With SECOND the
// second product's accumulators end in part [n_out][d].
template <int CT, int DT, bool SECOND, class Setup, class Rows, class Column>
__device__ __forceinline__ void row_tile_sweep(float *lds, const float *E, const int32_t *nodes, int64_t m, int ld, int d, int n_out, const float *W, int KW,
                                               float *part, Setup &setup, Rows &rows, Column &column) {
    typedef RowTiles<CT, DT, SECOND> T;
    constexpr int XS = T::XS, PS = T::PS, N1 = T::N1, N2 = T::N2, NPF = T::NPF;
    float *Xs = lds, *Ps = Xs + RT_ROWS * XS, *Ws = Ps + RT_ROWS * PS;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int WS = KW + 1;
    const bool resident = KW >= ld;
    const int64_t n_tiles = (m + RT_ROWS - 1) / RT_ROWS;

    auto stage_w = [&](int k0) {  // columns [k0, k0 + KW) of W -> Ws (rows behind n_out and columns behind d: zeros)
        const int kw = min(KW, ld - k0);
        for (int i = tid; i < 32 * CT * kw; i += 256) {
            const int c = i / kw, kk = i - c * kw, k = k0 + kk;
            Ws[c * WS + kk] = (c < n_out && k < d) ? W[(int64_t)c * d + k] : 0.f;
        }
    };
    float4 pf[NPF];
    auto fetch = [&](int64_t tile) {  // the tile's rows -> registers (rows behind M and columns behind ld: zeros)
        const int64_t row0 = tile * RT_ROWS;
#pragma unroll
        for (int j = 0; j < NPF; ++j) {
            const int i = tid + 256 * j, r = i / (8 * DT), col = (i % (8 * DT)) * 4;
            pf[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (tile < n_tiles && row0 + r < m && col < ld) pf[j] = *(const float4 *)(E + (int64_t)nodes[row0 + r] * ld + col);
        }
    };

    f32x16 acc2[N2];
#pragma unroll
    for (int i = 0; i < N2; ++i)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc2[i][q] = 0.f;

    fetch(blockIdx.x);
    if (resident) stage_w(0);
    setup((const float *)Ws, WS, resident);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = tile * RT_ROWS;
        __syncthreads();  // the previous tile's second product has read Xs / Ps
#pragma unroll
        for (int j = 0; j < NPF; ++j) {
            const int i = tid + 256 * j, r = i / (8 * DT), col = (i % (8 * DT)) * 4;
            float *x = Xs + r * XS + col;
            x[0] = pf[j].x; x[1] = pf[j].y; x[2] = pf[j].z; x[3] = pf[j].w;
        }
        fetch(tile + gridDim.x);
        if (resident) __syncthreads();

        // first product: unit u = wv + 4 i is (row half u & 1, output tile u >> 1)
        f32x16 acc1[N1];
#pragma unroll
        for (int i = 0; i < N1; ++i)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc1[i][q] = 0.f;
        for (int k0 = 0; k0 < ld; k0 += KW) {
            if (!resident) {
                __syncthreads();
                stage_w(k0);
                __syncthreads();
            }
            const int kmax = min(KW, ld - k0);
#pragma unroll
            for (int i = 0; i < N1; ++i) {
                const int u = wv + 4 * i;
                if (u < 2 * CT) {
                    const float *xa = Xs + ((u & 1) * 32 + l31) * XS + k0 + half;
                    const float *wb = Ws + ((u >> 1) * 32 + l31) * WS + half;
                    int kk = 0;
                    for (; kk + 16 <= kmax; kk += 16) {  // (8 steps: their 16 LDS reads are issued ahead of the matrix instructions)
                        float xv[8], wv8[8];
#pragma unroll
                        for (int s = 0; s < 8; ++s) {
                            xv[s] = xa[kk + 2 * s];
                            wv8[s] = wb[kk + 2 * s];
                        }
#pragma unroll
                        for (int s = 0; s < 8; ++s) acc1[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[s], wv8[s], acc1[i], 0, 0, 0);
                    }
                    for (; kk < kmax; kk += 2) acc1[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[kk], wb[kk], acc1[i], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < N1; ++i) {
            const int u = wv + 4 * i;
            if (u < 2 * CT) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) Ps[((u & 1) * 32 + tile_row(reg, half)) * PS + (u >> 1) * 32 + l31] = acc1[i][reg];
            }
        }
        __syncthreads();

        rows(row0, (const float *)Xs, Ps);

        // second product: tile t = wv + 4 i is (output tile t / DT, column tile t % DT); k runs over the 64 rows
        if constexpr (SECOND) {
            __syncthreads();
            if (tid < n_out) {
#pragma unroll 8
                for (int r = 0; r < RT_ROWS; ++r) column(Ps[r * PS + tid]);
            }
#pragma unroll
            for (int i = 0; i < N2; ++i) {
                const int t = wv + 4 * i;
                if (t < CT * DT) {
                    const float *pa = Ps + half * PS + (t / DT) * 32 + l31;
                    const float *xb = Xs + half * XS + (t % DT) * 32 + l31;
#pragma unroll 8
                    for (int k = 0; k < RT_ROWS; k += 2) acc2[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[k * PS], xb[k * XS], acc2[i], 0, 0, 0);
                }
            }
        }
    }

    if constexpr (SECOND) {
#pragma unroll
        for (int i = 0; i < N2; ++i) {
            const int t = wv + 4 * i;
            if (t < CT * DT) {
                const int col = (t % DT) * 32 + l31;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int c = (t / DT) * 32 + tile_row(reg, half);
                    if (c < n_out && col < d) part[(int64_t)c * d + col] = acc2[i][reg];
                }
            }
        }
    }
}

// The workgroup's 256 float64 terms `v`, added by a fixed tree in red[256], leave as out[0] = high part, out[1] = remainder.
// With redi: the 256 integers `vi` ride along in the same tree, their sum to *outi.
__device__ __forceinline__ void rt_block_sum(double *red, double v, float *out, int *redi = nullptr, int vi = 0, int32_t *outi = nullptr) {
    const int tid = threadIdx.x;
    red[tid] = v;
    if (redi) redi[tid] = vi;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            red[tid] += red[tid + w];
            if (redi) redi[tid] += redi[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float hi = (float)red[0];
        out[0] = hi;
        out[1] = (float)(red[0] - (double)hi);
        if (redi) *outi = redi[0];
    }
}

// ---- host side shared by classifier.hip and kmeans.hip ----

// The launch plan of a sweep: template instance, grid (a function of m alone), dynamic LDS and the W k-chunk.
struct RowTilePlan {
    int CT, DT, grid, KW;
    size_t lds;
};

inline RowTilePlan row_tile_plan(int64_t m, int n_out, int ld) {
    const int CT = cdiv(n_out, 32), DT = cdiv(ld, 32);
    const size_t fixed = sizeof(float) * RT_ROWS * ((size_t)(32 * DT + 1) + (32 * CT + 1));
    int KW = (int)((RT_LDS - fixed) / (sizeof(float) * 32 * CT)) - 1;
    KW = KW >= ld ? ld : (KW / 4) * 4;
    return RowTilePlan{CT, DT, (int)std::min<int64_t>(RT_MAX_GRID, (m + RT_ROWS - 1) / RT_ROWS), KW, fixed + sizeof(float) * 32 * CT * (size_t)(KW + 1)};
}

// The rows of a call: `which`, then the caller's own check of n_out (range: () -> GG_OK or its failure), then m, n_emb, the ids.
template <class Range>
int check_rows(gg_ctx *ctx, const char *fn, int which, const int32_t *nodes, int64_t m, Range range) {
    GG_CHECK(ctx, which == 0 || which == 1, GG_EINVAL, "%s: which must be 0 (generator) or 1 (discriminator), got %d", fn, which);
    if (const int rc = range()) return rc;
    GG_CHECK(ctx, m >= 1 && m <= 0x7fffffffLL, GG_EINVAL, "%s: m = %lld outside [1, 2^31 - 1]", fn, (long long)m);
    GG_CHECK(ctx, ctx->n_emb <= RT_MAX_D, GG_EINVAL, "%s: supports n_emb <= %d (got %d)", fn, RT_MAX_D, ctx->n_emb);
    GG_CHECK(ctx, nodes != nullptr, GG_EINVAL, "%s: nodes is NULL", fn);
    for (int64_t i = 0; i < m; ++i)
        GG_CHECK(ctx, nodes[i] >= 0 && nodes[i] < ctx->n_node, GG_EINVAL, "%s: node id %d (entry %lld) outside [0, %d)", fn, nodes[i], (long long)i, ctx->n_node);
    return GG_OK;
}

}  // namespace gg
