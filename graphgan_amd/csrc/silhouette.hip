// silhouette.hip -- exact silhouette of a node partition: for every evaluated row the mean Euclidean distance to the rows of
// its own cluster (a) and to those of the nearest other cluster (b), over ALL pairs.  The fourth consumer of the tile stream
// (score_tiles.h): the stream gives s_ij = x_i . x_j in registers, the distance is sqrtf(max(0, (h_i + h_j) - 2 s_ij)) with
// h = |x|^2, and the consumer keeps one running sum per (row, cluster).  Nothing of size m x m or m x n_emb exists on the host.
//
// What makes the sum order fixed without atomics is a CLUSTER-SORTED COPY of the set:
//   - the host sorts the positions by (cluster, node id) and gives every cluster a segment of the copy padded to a multiple of
//     32 rows, so that every 32-column tile a wavefront receives belongs to exactly one cluster (tile_cluster / tile_valid:
//     the cluster and the number of real rows of each tile);
//   - the copy (fp32 [M', ld], or for bf16 the tiled form of bf16_piece, both gathered from the resident table; pad rows are
//     zeros) is BOTH operands of the stream: requested rows are positions into it, the streamed columns are all of it.  The
//     producers f32_score_tiles and bf16_score_tiles run unchanged;
//   - the consumer adds the distances of the tiles of one cluster into 16 sums per lane (one per accumulator row; pad columns
//     and the row's own position masked to +0), and when the tile's cluster changes, and at the end of the workgroup's
//     column split, folds the 32 lanes of each half-wave by a butterfly and writes ONE partial per (split, wavefront, row,
//     cluster) to a stage (zeroed in front of the pass: a wavefront that never met a cluster contributes +0);
//   - sil_finish_kernel adds a (row, cluster)'s partials in ascending (split, wavefront) order, divides, takes the minimum
//     with ties to the lowest cluster and writes sil / a / b / nearest.
// The column split depends on the SET alone (m and the padded size M'), never on how many rows are requested, and neither a
// lane's sum nor the fold depends on which accumulator register or half-wave holds a row: a row's outputs are the same bits
// whether it is evaluated with all rows or in a sample, and in whichever order the caller lists the set.
// The stage is bounded: the requested rows go through in passes of at most SIL_CHUNK rows, fewer where splits x 4 x k
// partials per row would exceed SIL_STAGE_BYTES (as rank_score.hip bounds its passes with RK_CHUNK).
#include <math.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "score_tiles.h"

namespace gg {

namespace {

constexpr int SIL_CHUNK = 4096;                  // requested rows per internal pass at most
constexpr size_t SIL_STAGE_BYTES = 64u << 20;    // the (split, wavefront, cluster, row) stage of a pass at most
constexpr int SIL_MAX_SPLITS = 32;

struct SilArgs {
    const int32_t *pos;           // [n] the pass's requested rows: positions into the copy
    int n;
    const float *h;               // [M'] |x|^2 of every copy row (pad rows: 0)
    const int32_t *tile_cluster;  // [M' / 32] cluster of the tile's rows
    const int32_t *tile_valid;    // [M' / 32] real rows of the tile (1 .. 32), the pad rows behind them
    int k;
    float *part;                  // [splits * 4][k][chunk] partial sums of the pass
    int chunk;
};

// the fp32 copy [n_rows, ld]: row p = E[src[p]], zeros where src[p] < 0
__global__ __launch_bounds__(256) void sil_gather_kernel(const float *E, int ld, const int32_t *src, int64_t n_quads, float *X) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_quads) return;
    const int q = ld / 4;
    const int64_t p = i / q;
    const int kk = (int)(i % q) * 4;
    const int node = src[p];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (node >= 0) v = *(const float4 *)(E + (int64_t)node * ld + kk);
    *(float4 *)(X + p * ld + kk) = v;
}

// the gathering variant of all_score.hip's to_bf16_kernel: one 16-byte piece of the tiled bf16 copy per thread (piece index as
// bf16_piece: ((tile * KS + s) * 64 + 32 h + r % 32), k = 16 s + 8 h .. + 8 of copy row r = E[src[r]], zeros behind ld and for pads
__global__ __launch_bounds__(256) void sil_tile_bf16_kernel(const float *E, int ld, const int32_t *src, int KS, int64_t n_pieces, uint4 *Xb) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pieces) return;
    const int64_t tile = i / (KS * 64);
    const int s = (int)((i >> 6) % KS), half = (int)(i >> 5) & 1;
    const int node = src[tile * 32 + (i & 31)];
    const int k0 = 16 * s + 8 * half;
    union { uint4 u; bf16x8 v; } f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float x = (node >= 0 && k0 + j < ld) ? E[(int64_t)node * ld + k0 + j] : 0.f;
        f.v[j] = (__bf16)x;
    }
    Xb[i] = f.u;
}

// The consumer handed to the producers of score_tiles.h: per lane, for the 16 rows it holds (tile_row(reg, lane >> 5)), the
// row's copy position and |x|^2 and the running sum of distances to the columns of the current cluster.
struct SilConsumer {
    float hr[16], sum[16];
    int rp[16];
    int cur;  // cluster of the running sums (wavefront-uniform), -1: none yet
    const SilArgs &o;
    const int r0, split, tile_end;
    __device__ __forceinline__ SilConsumer(const SilArgs &o_, int r0_, int split_, int tile_end_) : o(o_), r0(r0_), split(split_), tile_end(tile_end_) {}
    __device__ __forceinline__ void init() {
        const int half = (threadIdx.x & 63) >> 5;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = r0 + tile_row(reg, half);
            const int p = row < o.n ? o.pos[row] : -1;  // (rows behind the pass match no column and are never written)
            rp[reg] = p;
            hr[reg] = p >= 0 ? o.h[p] : 0.f;
            sum[reg] = 0.f;
        }
        cur = -1;
    }
    __device__ __forceinline__ float start(int, bool) const { return 0.f; }
    // the sums of cluster `cur`: folded over the 32 lanes of each half-wave (lanes l and l ^ 32 hold different rows) by a
    // butterfly -- the same tree for every register and both halves --, one partial per row written, the sums cleared
    __device__ __forceinline__ void flush() {
        if (cur < 0) return;
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        float *dst = o.part + ((size_t)(split * 4 + wv) * o.k + cur) * o.chunk;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            float v = sum[reg];
#pragma unroll
            for (int off = 16; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
            const int row = r0 + tile_row(reg, lane >> 5);
            if ((lane & 31) == 0 && row < o.n) dst[row] = v;
            sum[reg] = 0.f;
        }
    }
    __device__ __forceinline__ void operator()(const f32x16 &acc, int col, bool) {
        const int tile = __builtin_amdgcn_readfirstlane(col >> 5);  // (a wavefront's 32 columns are one tile of the copy)
        if (tile >= tile_end) return;                               // behind the split's end
        const int c = o.tile_cluster[tile], valid = o.tile_valid[tile];
        if (c != cur) {
            flush();
            cur = c;
        }
        const float hc = o.h[col];
        const bool live = (col & 31) < valid;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const float d2 = (hr[reg] + hc) - 2.f * acc[reg];
            const float d = __builtin_sqrtf(fmaxf(0.f, d2));
            sum[reg] += (live && col != rp[reg]) ? d : 0.f;  // the own term is dropped by position
        }
    }
    __device__ __forceinline__ void operator()(const f32x16 (&acc)[1], int col, bool ok) { (*this)(acc[0], col, ok); }
    __device__ __forceinline__ void finish() { flush(); }
};

// Launch shapes of rank_f32_kernel / rank_bf16_kernel: grid = (column splits, 32-row tiles), 4 wavefronts of 32 columns each.
// n_cols = M' is a multiple of 32 and cols_per_split one of 128, so every split ends on a tile boundary.
__global__ __launch_bounds__(256) void sil_f32_kernel(const float *X, int n_cols, int ld, int cols_per_split, SilArgs o) {
    extern __shared__ float As_all[];  // [32][ld + 1]: the tile's 32 requested rows, staged once
    __shared__ float Bs[128][ST_KC + 1];
    const int split = blockIdx.x, r0 = blockIdx.y * 32;
    const int cbeg = split * cols_per_split, cend = min(n_cols, cbeg + cols_per_split);
    SilConsumer sums(o, r0, split, cend >> 5);
    f32_score_tiles(X, ld, o.pos, o.n, r0, cbeg, cend, As_all, Bs, sums);
    sums.finish();
}

template <int KS>
__global__ __launch_bounds__(256) void sil_bf16_kernel(const uint4 *Xb, int n_cols, int cols_per_split, SilArgs o) {
    const int split = blockIdx.x, r0 = blockIdx.y * 32;
    const int cbeg = split * cols_per_split, cend = min(n_cols, cbeg + cols_per_split);
    SilConsumer sums(o, r0, split, cend >> 5);
    bf16_score_tiles<KS, 1, (KS <= 16)>(Xb, o.pos, o.n, r0, cbeg, cend, sums);
    sums.finish();
}

// One thread per requested row of the pass: S_ic = the partials of (row, c) added in ascending (split, wavefront) order, then
// the divisions, the minimum over the other non-empty clusters (strict <: ties to the lowest c) and sil.
__global__ __launch_bounds__(256) void sil_finish_kernel(SilArgs o, int n_parts, const int32_t *counts, float *sil, float *a_out, float *b_out,
                                                         int32_t *nearest) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= o.n) return;
    const int own = o.tile_cluster[o.pos[r] >> 5];
    float a = 0.f, b = INFINITY;
    int bc = -1;
    for (int c = 0; c < o.k; ++c) {
        const int nc = counts[c];
        if (nc == 0) continue;
        float S = 0.f;
        for (int sw = 0; sw < n_parts; ++sw) S += o.part[((size_t)sw * o.k + c) * o.chunk + r];
        if (c == own) {
            a = nc > 1 ? S / (float)(nc - 1) : 0.f;
        } else {
            const float mean = S / (float)nc;
            if (mean < b || bc < 0) {
                b = mean;
                bc = c;
            }
        }
    }
    const float den = fmaxf(a, b);
    sil[r] = (counts[own] == 1 || den == 0.f) ? 0.f : (b - a) / den;
    a_out[r] = a;
    b_out[r] = b;
    nearest[r] = bc;
}

}  // namespace

}  // namespace gg

using namespace gg;

// gg_silhouette: see include/graphgan_hip.h.
extern "C" int gg_silhouette(gg_ctx *ctx, int which, const int32_t *nodes, const int32_t *assign, int64_t m, int k, const int64_t *rows, int64_t n_rows,
                             int precision, float *sil_out, float *a_out, float *b_out, int32_t *nearest_out, double *mean_out, double *ms_out) {
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    GG_CHECK(ctx, which == 0 || which == 1, GG_EINVAL, "gg_silhouette: which must be 0 (generator) or 1 (discriminator)");
    GG_CHECK(ctx, precision == 0 || precision == 1, GG_EINVAL, "gg_silhouette: precision must be 0 (fp32) or 1 (bf16)");
    GG_CHECK(ctx, nodes && assign, GG_EINVAL, "gg_silhouette: bad argument");
    GG_CHECK(ctx, k >= 2 && k <= 128, GG_EINVAL, "gg_silhouette: k = %d outside [2, 128]", k);
    GG_CHECK(ctx, m >= 2 && m <= 0x7fffffffLL, GG_EINVAL, "gg_silhouette: m = %lld outside [2, 2^31 - 1]", (long long)m);
    GG_CHECK(ctx, !rows || (n_rows >= 1 && n_rows <= 0x7fffffffLL), GG_EINVAL, "gg_silhouette: n_rows = %lld outside [1, 2^31 - 1]", (long long)n_rows);
    const int n = ctx->n_node, ld = ctx->ld;
    GG_CHECK(ctx, precision == 0 || ctx->n_emb <= 512, GG_EINVAL, "gg_silhouette: bf16 supports n_emb <= 512 (got %d)", ctx->n_emb);
    const size_t dyn = sizeof(float) * 32 * (size_t)(ld + 1);
    GG_CHECK(ctx, precision == 1 || dyn <= 140 * 1024, GG_EINVAL, "gg_silhouette: fp32 supports n_emb <= 1116 (got %d)", ctx->n_emb);
    if (ms_out) *ms_out = 0.0;
    std::vector<int32_t> counts(k, 0);
    for (int64_t i = 0; i < m; ++i) {
        GG_CHECK(ctx, nodes[i] >= 0 && nodes[i] < n, GG_EINVAL, "gg_silhouette: nodes[%lld] = %d out of range [0, %d)", (long long)i, nodes[i], n);
        GG_CHECK(ctx, assign[i] >= 0 && assign[i] < k, GG_EINVAL, "gg_silhouette: assign[%lld] = %d outside [0, k = %d)", (long long)i, assign[i], k);
        ++counts[assign[i]];
    }
    {
        std::vector<uint8_t> seen(n, 0);
        for (int64_t i = 0; i < m; ++i) {
            GG_CHECK(ctx, !seen[nodes[i]], GG_EINVAL, "gg_silhouette: node id %d is repeated (nodes[%lld])", nodes[i], (long long)i);
            seen[nodes[i]] = 1;
        }
    }
    if (rows)
        for (int64_t t = 0; t < n_rows; ++t)
            GG_CHECK(ctx, rows[t] >= 0 && rows[t] < m, GG_EINVAL, "gg_silhouette: rows[%lld] = %lld outside [0, m = %lld)", (long long)t, (long long)rows[t],
                     (long long)m);
    const int n_full = (int)std::count_if(counts.begin(), counts.end(), [](int32_t c) { return c > 0; });
    GG_CHECK(ctx, n_full >= 2, GG_EINVAL, "gg_silhouette: %d non-empty cluster(s), at least 2 are needed", n_full);
    // the copy's layout: cluster c at [seg[c], seg[c] + counts[c]), padded to a multiple of 32 rows
    std::vector<int64_t> seg(k + 1, 0);
    for (int c = 0; c < k; ++c) seg[c + 1] = seg[c] + ((int64_t)counts[c] + 31) / 32 * 32;
    const int64_t Mp64 = seg[k];
    GG_CHECK(ctx, Mp64 <= 0x7fffff00LL, GG_EINVAL, "gg_silhouette: the padded set of %lld rows is outside [2, 2^31 - 256]", (long long)Mp64);
    const int Mp = (int)Mp64, n_tiles = Mp / 32;
    std::vector<int64_t> order(m);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return assign[x] != assign[y] ? assign[x] < assign[y] : nodes[x] < nodes[y]; });
    std::vector<int32_t> src(Mp, -1), pos_of(m), tile_cluster(n_tiles), tile_valid(n_tiles);
    {
        int64_t j = 0;
        for (int c = 0; c < k; ++c) {
            for (int32_t i = 0; i < counts[c]; ++i, ++j) {
                src[seg[c] + i] = nodes[order[j]];
                pos_of[order[j]] = (int32_t)(seg[c] + i);
            }
            for (int64_t t = seg[c] / 32; t < seg[c + 1] / 32; ++t) {
                tile_cluster[t] = c;
                tile_valid[t] = (int32_t)std::min<int64_t>(32, counts[c] - (t * 32 - seg[c]));
            }
        }
    }
    // the requested rows: distinct copy positions, ascending; slot[position] = its place among them
    const int64_t n_out = rows ? n_rows : m;
    std::vector<int32_t> req;
    if (rows) {
        req.resize(n_rows);
        for (int64_t t = 0; t < n_rows; ++t) req[t] = pos_of[rows[t]];
        std::sort(req.begin(), req.end());
        req.erase(std::unique(req.begin(), req.end()), req.end());
    } else {
        req.reserve(m);
        for (int p = 0; p < Mp; ++p)
            if (src[p] >= 0) req.push_back(p);
    }
    const int64_t n_req = (int64_t)req.size();
    // the column split is a function of the set alone
    const ColumnSplit cs = column_split(Mp, cdiv(std::min<int64_t>(m, SIL_CHUNK), 32), 2048, SIL_MAX_SPLITS);
    const int n_parts = cs.splits * 4;
    const size_t per_row = sizeof(float) * (size_t)n_parts * k;
    int chunk = (int)std::min<size_t>(SIL_CHUNK, SIL_STAGE_BYTES / per_row) / 32 * 32;
    chunk = std::max(32, chunk);
    chunk = (int)std::min<int64_t>(chunk, (n_req + 31) / 32 * 32);
    const Bf16Shape bs = bf16_shape(ctx->n_emb);
    const Model &M = ctx->model[which];

    GG_HIP(ctx, hipSetDevice(ctx->device));
    ScopedBuf d_src, d_tc, d_tv, d_cnt, d_req, d_h, d_x, d_part, d_sil, d_a, d_b, d_near;
    hipError_t e = d_src.reserve(sizeof(int32_t) * (size_t)Mp);
    if (e == hipSuccess) e = d_tc.reserve(sizeof(int32_t) * n_tiles);
    if (e == hipSuccess) e = d_tv.reserve(sizeof(int32_t) * n_tiles);
    if (e == hipSuccess) e = d_cnt.reserve(sizeof(int32_t) * k);
    if (e == hipSuccess) e = d_req.reserve(sizeof(int32_t) * (size_t)n_req);
    if (e == hipSuccess) e = d_h.reserve(sizeof(float) * (size_t)Mp);
    if (e == hipSuccess) e = d_x.reserve(precision == 0 ? sizeof(float) * (size_t)Mp * ld : sizeof(uint4) * (size_t)n_tiles * bs.KS * 64);
    if (e == hipSuccess) e = d_part.reserve(per_row * chunk);
    if (e == hipSuccess) e = d_sil.reserve(sizeof(float) * (size_t)n_req);
    if (e == hipSuccess) e = d_a.reserve(sizeof(float) * (size_t)n_req);
    if (e == hipSuccess) e = d_b.reserve(sizeof(float) * (size_t)n_req);
    if (e == hipSuccess) e = d_near.reserve(sizeof(int32_t) * (size_t)n_req);
    if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "gg_silhouette: %s", hipGetErrorString(e));
    std::vector<float> h_sil(n_req), h_a(n_req), h_b(n_req);
    std::vector<int32_t> h_near(n_req);
    hipStream_t st = ctx->stream;
    e = hipMemcpyAsync(d_src.p, src.data(), sizeof(int32_t) * (size_t)Mp, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tc.p, tile_cluster.data(), sizeof(int32_t) * n_tiles, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tv.p, tile_valid.data(), sizeof(int32_t) * n_tiles, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_cnt.p, counts.data(), sizeof(int32_t) * k, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_req.p, req.data(), sizeof(int32_t) * (size_t)n_req, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        (void)hipEventRecord(ctx->ev0, st);
        const dim3 rgrid(cdiv(Mp, 256));
        if (precision == 0) {
            const int64_t n_quads = (int64_t)Mp * (ld / 4);
            hipLaunchKernelGGL(sil_gather_kernel, dim3((unsigned)((n_quads + 255) / 256)), dim3(256), 0, st, M.E, ld, d_src.as<int32_t>(), n_quads, d_x.as<float>());
            hipLaunchKernelGGL(sil_norm_kernel<false>, rgrid, dim3(256), 0, st, M.E, ld, d_src.as<int32_t>(), Mp, d_h.as<float>());
            if (dyn > 48 * 1024) (void)hipFuncSetAttribute((const void *)sil_f32_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
        } else {
            const int64_t n_pieces = (int64_t)n_tiles * bs.KS * 64;
            hipLaunchKernelGGL(sil_tile_bf16_kernel, dim3((unsigned)((n_pieces + 255) / 256)), dim3(256), 0, st, M.E, ld, d_src.as<int32_t>(), bs.KS, n_pieces,
                               d_x.as<uint4>());
            hipLaunchKernelGGL(sil_norm_kernel<true>, rgrid, dim3(256), 0, st, M.E, ld, d_src.as<int32_t>(), Mp, d_h.as<float>());
        }
        e = hipGetLastError();
    }
    for (int64_t c0 = 0; c0 < n_req && e == hipSuccess; c0 += chunk) {
        const int cr = (int)std::min<int64_t>(chunk, n_req - c0);
        e = hipMemsetAsync(d_part.p, 0, per_row * chunk, st);
        if (e != hipSuccess) break;
        SilArgs o{d_req.as<int32_t>() + c0, cr, d_h.as<float>(), d_tc.as<int32_t>(), d_tv.as<int32_t>(), k, d_part.as<float>(), chunk};
        const dim3 grid(cs.splits, cdiv(cr, 32));
        if (precision == 0) hipLaunchKernelGGL(sil_f32_kernel, grid, dim3(256), dyn, st, d_x.as<float>(), Mp, ld, cs.cols_per_split, o);
        else if (bs.KS == 4) hipLaunchKernelGGL(sil_bf16_kernel<4>, grid, dim3(256), 0, st, d_x.as<uint4>(), Mp, cs.cols_per_split, o);
        else if (bs.KS == 8) hipLaunchKernelGGL(sil_bf16_kernel<8>, grid, dim3(256), 0, st, d_x.as<uint4>(), Mp, cs.cols_per_split, o);
        else if (bs.KS == 16) hipLaunchKernelGGL(sil_bf16_kernel<16>, grid, dim3(256), 0, st, d_x.as<uint4>(), Mp, cs.cols_per_split, o);
        else hipLaunchKernelGGL(sil_bf16_kernel<32>, grid, dim3(256), 0, st, d_x.as<uint4>(), Mp, cs.cols_per_split, o);
        hipLaunchKernelGGL(sil_finish_kernel, dim3(cdiv(cr, 256)), dim3(256), 0, st, o, n_parts, d_cnt.as<int32_t>(), d_sil.as<float>() + c0,
                           d_a.as<float>() + c0, d_b.as<float>() + c0, d_near.as<int32_t>() + c0);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        (void)hipEventRecord(ctx->ev1, st);
        e = hipMemcpyAsync(h_sil.data(), d_sil.p, sizeof(float) * (size_t)n_req, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_a.data(), d_a.p, sizeof(float) * (size_t)n_req, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_b.data(), d_b.p, sizeof(float) * (size_t)n_req, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_near.data(), d_near.p, sizeof(int32_t) * (size_t)n_req, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);  // (also on a failed path: the buffers are freed behind it)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(ctx, GG_EHIP, "gg_silhouette: %s", hipGetErrorString(e));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    if (ms_out) *ms_out = ms;
    // to output order; the mean is the float64 sum of sil in that order
    std::vector<int32_t> slot(Mp, -1);
    for (int64_t j = 0; j < n_req; ++j) slot[req[j]] = (int32_t)j;
    double total = 0.0;
    for (int64_t t = 0; t < n_out; ++t) {
        const int32_t j = slot[pos_of[rows ? rows[t] : t]];
        if (sil_out) sil_out[t] = h_sil[j];
        if (a_out) a_out[t] = h_a[j];
        if (b_out) b_out[t] = h_b[j];
        if (nearest_out) nearest_out[t] = h_near[j];
        total += (double)h_sil[j];
    }
    if (mean_out) *mean_out = total / (double)n_out;
    return GG_OK;
}
