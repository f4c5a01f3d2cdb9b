// score_tiles.h -- the matrix-core tile stream over S = E_rows . E^T, written once for its two users: the streamed all-pairs
// consumer (all_score.hip: max / argmax / log-sum-exp per row) and the top-K consumer (topk_score.hip: k-lists per row).
// A PRODUCER walks the columns [cbeg, cend) of a workgroup's split in 128-column tiles -- its 4 wavefronts take 32 columns
// each -- and hands every finished 32 x 32 accumulator to a CONSUMER object, in registers.  Producers and consumers are
// __forceinline__ throughout: a consumer behind a call, or in scratch, fails the build's audit (check_no_scratch.sh).
// Behind the device part: the host plan both entry points share (definitions in all_score.hip).
#pragma once
#include "gg_internal.h"

namespace gg {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int ST_KC = 32;  // k-chunk of the fp32 tile staging

// C/D layout of v_mfma_f32_32x32x*: accumulator register `reg` of a lane in half-wave `half` (= lane >> 5) holds
// column lane & 31 of this row of the tile
__device__ __forceinline__ int tile_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

// The bf16 copy of a table (round to nearest even, k zero padded to ld16 = 16 KS, rows zero padded to a multiple of 32) is
// TILED for the matrix instruction's B operand: the 16-byte piece {k = 16 s + 8 h .. + 8} of row r sits at piece index
//     ((r / 32) * KS + s) * 64 + 32 h + r % 32,
// i.e. the 64 lanes of a wavefront that loads k-step s of a 32-column tile (lane = 32 h + column) read ONE CONTIGUOUS KILOBYTE.
// (Row-major, every such load touched 32 different cache lines for 32 bytes each: 4 wavefronts x 16 loads x 32 line look-ups per
// tile and CU were what the wide consumer waited for, not the HBM and not the matrix pipe.)
__device__ __forceinline__ int64_t bf16_piece(int64_t r, int s, int h, int KS) { return ((r >> 5) * KS + s) * 64 + 32 * h + (r & 31); }

// fp32 stream: v_mfma_f32_32x32x2_f32, bit-for-bit a k-ordered fmaf chain from 0.0 (the arithmetic of gg_all_score).  The
// tile's 32 requested rows (rows[r0 ..], or r0 .. when rows is NULL) are staged ONCE into As_all[32][ld + 1], 128 table rows per
// k-chunk into Bs; behind the staging the consumer sets itself up (consume.init()), then every finished tile goes to
// consume(acc, col, col < cend).
template <class Consume>
__device__ __forceinline__ void f32_score_tiles(const float *E, int ld, const int32_t *rows, int n_rows, int r0, int cbeg, int cend,
                                                float *As_all, float (*Bs)[ST_KC + 1], Consume &consume) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int lda = ld + 1;
    for (int i = tid; i < 32 * (ld / 4); i += 256) {
        const int r = i / (ld / 4), kk = (i % (ld / 4)) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r0 + r < n_rows) {
            const int node = rows ? rows[r0 + r] : r0 + r;
            v = *(const float4 *)(E + (int64_t)node * ld + kk);
        }
        float *d = As_all + r * lda + kk;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    consume.init();
    for (int c0 = cbeg; c0 < cend; c0 += 128) {
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        for (int k0 = 0; k0 < ld; k0 += ST_KC) {
            __syncthreads();  // also orders the A staging before its first use
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = (tid >> 3) + 32 * i, kk = (tid & 7) * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c0 + r < cend && k0 + kk < ld) v = *(const float4 *)(E + (int64_t)(c0 + r) * ld + k0 + kk);
                Bs[r][kk] = v.x; Bs[r][kk + 1] = v.y; Bs[r][kk + 2] = v.z; Bs[r][kk + 3] = v.w;
            }
            __syncthreads();
            const int kmax = min(ST_KC, ld - k0);
            for (int kk = 0; kk < kmax; kk += 2) {
                const float a = As_all[(lane & 31) * lda + k0 + kk + (lane >> 5)];
                const float b = Bs[wv * 32 + (lane & 31)][kk + (lane >> 5)];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
            }
        }
        const int col = c0 + wv * 32 + (lane & 31);
        consume(acc, col, col < cend);
    }
}

// Narrow bf16 stream: v_mfma_f32_32x32x16_bf16 on the tiled copy Eb, KS = ld16 / 16 k-steps, RB blocks of 32 requested rows per
// workgroup.  No LDS for the operands: the A fragments of the rows stay in registers for the whole column sweep, every lane
// streams the 8-element k-slices of its own column straight from the copy (16 bytes per load; the two half-waves read the two
// halves of a 32-byte piece).  PF: the B fragments are double buffered in registers -- the KS loads of the NEXT tile are issued
// before the matrix instructions and the consumer of the current one, so that memory latency hides behind them.
// consume.init() runs behind the loads of the A fragments; the accumulators of a column start at consume.start(col, ok); every
// finished tile goes to consume(acc[RB], col, ok).
template <int KS, int RB, bool PF, class Consume>
__device__ __forceinline__ void bf16_score_tiles(const uint4 *Eb, const int32_t *rows, int n_rows, int r0, int cbeg, int cend, Consume &consume) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, half = lane >> 5;
    union Frag { uint4 u; bf16x8 v; };
    Frag afrag[RB][KS];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const int r = r0 + rb * 32 + (lane & 31);
        const int node = r < n_rows ? (rows ? rows[r] : r) : -1;
#pragma unroll
        for (int s = 0; s < KS; ++s) afrag[rb][s].u = node >= 0 ? Eb[bf16_piece(node, s, half, KS)] : make_uint4(0u, 0u, 0u, 0u);
    }
    consume.init();
    Frag bcur[KS], bnxt[PF ? KS : 1];
    auto load_tile = [&](Frag *dst, int c0t) {
        // (tiles start at multiples of 32 columns; the padded rows behind the table's end are zeros; a prefetch behind the
        // split's end re-reads its first tile)
        const uint4 *brow = Eb + (int64_t)((c0t < cend ? c0t : cbeg) >> 5) * KS * 64 + lane;
#pragma unroll
        for (int s = 0; s < KS; ++s) dst[s].u = brow[64 * s];
    };
    if (PF) load_tile(bcur, cbeg + wv * 32);
    for (int c0 = cbeg + wv * 32; c0 < cend; c0 += 128) {
        const int col = c0 + (lane & 31);
        const bool ok = col < cend;
        if (PF) load_tile(bnxt, c0 + 128);
        else load_tile(bcur, c0);
        const float x0 = consume.start(col, ok);
        f32x16 acc[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[rb][i] = x0;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afrag[rb][s].v, bcur[s].v, acc[rb], 0, 0, 0);
        }
        if (PF) {
#pragma unroll
            for (int s = 0; s < KS; ++s) bcur[s] = bnxt[PF ? s : 0];
        }
        consume(acc, col, ok);
    }
}

// |x|^2 as the stream computes x . x in fp32: the k-ordered fmaf chain from 0.0 -- over the bf16-rounded row when BF.  Row p of the
// output is table row src[p] (src == NULL: row p itself); src[p] < 0 gives 0.  Shared by the silhouette (silhouette.hip: the rows
// of its cluster-sorted copy; the kernel keeps the name of this first user, which the build's audit counts) and the metric top-K
// (topk_score.hip: every table row).
template <bool BF>
__global__ __launch_bounds__(256) void sil_norm_kernel(const float *E, int ld, const int32_t *src, int n_rows, float *h) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_rows) return;
    const int node = src ? src[p] : p;
    float acc = 0.f;
    if (node >= 0) {
        const float *x = E + (int64_t)node * ld;
        for (int kk = 0; kk < ld; kk += 4) {
            float4 v = *(const float4 *)(x + kk);
            if (BF) { v.x = (float)(__bf16)v.x; v.y = (float)(__bf16)v.y; v.z = (float)(__bf16)v.z; v.w = (float)(__bf16)v.w; }
            acc = __builtin_fmaf(v.x, v.x, acc);
            acc = __builtin_fmaf(v.y, v.y, acc);
            acc = __builtin_fmaf(v.z, v.z, acc);
            acc = __builtin_fmaf(v.w, v.w, acc);
        }
    }
    h[p] = acc;
}

// ---- host plan shared by gg_all_score, gg_all_score_reduce and gg_topk_scores (all_score.hip) ----

// every rows[i] in [0, n_node), or GG_EINVAL "<entry>: row id .. out of range" (rows == NULL: all rows, nothing to check)
int check_row_ids(gg_ctx *ctx, const char *entry, const int32_t *rows, int n_rows);

// bf16: k-steps of 16 elements; the kernels are instantiated for KS = 4 / 8 / 16 / 32 of them, the copy is zero padded to ld16 = 16 KS
struct Bf16Shape {
    int KS, ld16;
};
Bf16Shape bf16_shape(int n_emb);

// enough workgroups for the chip: the columns are split (multiples of 128 columns per split) when there are few row tiles,
// into at most max_splits parts
struct ColumnSplit {
    int splits, cols_per_split;
};
ColumnSplit column_split(int n_node, int row_tiles, int target_workgroups, int max_splits = 0x7fffffff);

// reserves `buf` and fills it, on ctx->stream, with the tiled bf16 copy of model[which].E; a failed reservation is returned
hipError_t bf16_table(gg_ctx *ctx, int which, int ld16, DevBuf &buf);

}  // namespace gg
