// pretrain.hip -- skip-gram pre-training rows on the device (gg_pretrain_set_noise / gg_prepare_pretrain):
//   uniform or node2vec-biased random walks over the resident CSR -> window pairs -> negative samples -> (center, neighbor, label) rows
// in the buffers gg_d_pass trains the discriminator's table on (one-table skip-gram with negative sampling).  The reference
// has no counterpart: its pre_train/*.emb files come from an external DeepWalk / node2vec run (src/GraphGAN/config.py:33-34).
// The sampling contract P1-P5 with the biased walk P2b (include/graphgan_hip.h) is exact integer arithmetic on the Philox uniforms of gg_arith.h, so
// the rows do not depend on how the walks are spread over threads, waves or calls.  Nothing of size rows x 12 B crosses PCIe.
//
//   pt_walk_kernel    a thread per walk: walk_len dependent rowptr / col gathers (latency bound; parallel over the walks)
//   pt_walk_bias_kernel  the node2vec walk of P2b (gg_pretrain_set_walk_bias with unequal weights): a thread per walk, up to 32
//                     rejection trials per hop (a col gather and a binary search in the sorted list of the previous node each);
//                     the hops whose trials all fail are drawn exactly by the whole wavefront, one such lane after the other
//   pt_count_kernel   rows of each walk from its length -> device_exclusive_scan -> row offsets
//   pt_fill_kernel    a wavefront per walk: path and per-centre pair offsets in LDS, lanes over the walk's rows, one Philox draw
//                     and one search in the uint64 prefix sums per negative row, coalesced 4-byte stores
#include <algorithm>
#include <vector>

#include "gg_arith.h"
#include "gg_internal.h"

namespace gg {

constexpr int PT_MAX_LEN = 256, PT_MAX_WINDOW = 16, PT_MAX_NEG = 64;
constexpr int PT_WAVES = 4;        // walks (wavefronts) per workgroup of the fill kernel
constexpr int PT_SAMPLE = 2048;    // entries of the prefix-sum subsample the fill kernel keeps in LDS (16 KB)
constexpr int H_PT_TOTAL = gg_ctx::H_TOTAL + 8;  // pinned word of the row total (gg_prepare_g's H_TOTAL may belong to a begun launch)

// P3: pairs of centre i on a path of len nodes
__host__ __device__ __forceinline__ int pt_pairs_of(int i, int len, int window) {
    const int back = i < window ? i : window, fwd = len - 1 - i < window ? len - 1 - i : window;
    return back + fwd;
}

static int64_t pt_pairs_of_path(int len, int window) {
    int64_t c = 0;
    for (int i = 0; i < len; ++i) c += pt_pairs_of(i, len, window);
    return c;
}

// P1 + P2.  paths[g * walk_len + h], -1 behind the walk's end; walk g = (start index, w) = (g / wps, g % wps).
__global__ __launch_bounds__(256) void pt_walk_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                      const int32_t *__restrict__ starts, int64_t n_walks, int wps, int walk_len,
                                                      uint64_t seed, uint32_t stream, int32_t *__restrict__ paths,
                                                      int32_t *__restrict__ path_len) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_walks) return;
    const int64_t si = g / wps;
    const uint32_t w = (uint32_t)(g - si * wps);
    const int32_t s = starts[si];
    int32_t *p = paths + g * walk_len;
    int32_t cur = s;
    int len = 1;
    p[0] = s;
    for (int h = 1; h < walk_len; ++h) {
        const int64_t e0 = rowptr[cur], k = rowptr[cur + 1] - e0;
        if (k == 0) break;
        const uint64_t m = uniform53(seed, stream, (uint32_t)s, w, (uint32_t)h);
        cur = col[e0 + (int64_t)threshold(m, (uint64_t)k)];
        p[h] = cur;
        len = h + 1;
    }
    for (int h = len; h < walk_len; ++h) p[h] = -1;
    path_len[g] = len;
}

// P2b: the class weight of candidate x at a hop whose previous node is prev; sadj + [pe0, pe0 + pk) = the sorted list of prev.
struct PtBias {
    uint32_t w_ret, w_com, w_out, w_max;
};

__device__ __forceinline__ uint32_t pt_class_of(int32_t x, int32_t prev, const int32_t *__restrict__ sadj, int64_t pe0, int32_t pk,
                                                const PtBias &b) {
    if (x == prev) return b.w_ret;
    int32_t lo = 0, hi = pk;  // the first entry >= x
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (sadj[pe0 + mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo < pk && sadj[pe0 + lo] == x ? b.w_com : b.w_out;
}

constexpr int PT_TRIALS = 32;  // R of P2b

// P1 + P2b.  A lane per walk like pt_walk_kernel, but every lane of a wavefront stays in the hop loop until the last walk of
// the wavefront has ended (alive = 0 for the others): the exact draw behind PT_TRIALS rejections is made by all 64 lanes
// together -- __ballot names the lanes that need one, __shfl hands their state round -- so no thread ever scans a hub's list alone.
// The launch has whole wavefronts (256 threads a workgroup); lanes behind n_walks run along with valid = 0.
__global__ __launch_bounds__(256) void pt_walk_bias_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                           const int32_t *__restrict__ sadj, const int32_t *__restrict__ starts,
                                                           int64_t n_walks, int wps, int walk_len, uint64_t seed, uint32_t stream,
                                                           PtBias bias, int32_t *__restrict__ paths, int32_t *__restrict__ path_len) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = g < n_walks;
    const int64_t si = valid ? g / wps : 0;
    const uint32_t w = valid ? (uint32_t)(g - si * wps) : 0u;
    const int32_t s = valid ? starts[si] : 0;
    int32_t *p = paths + (valid ? g : 0) * walk_len;
    if (valid) p[0] = s;
    int32_t cur = s, prev = -1, pk = 0;
    int64_t pe0 = 0;  // the list of prev: the registers of the hop before
    int len = 1;
    bool alive = valid;
    for (int h = 1; h < walk_len; ++h) {
        if (__ballot(alive) == 0ull) break;  // (the same in every lane)
        int64_t e0 = 0;
        int32_t k = 0, nxt = -1;
        bool exhausted = false;
        if (alive) {
            e0 = rowptr[cur];
            k = (int32_t)(rowptr[cur + 1] - e0);
            if (k == 0) {
                alive = false;
            } else if (h == 1 || k == 1) {  // P2 (k == 1: t(1) = 0 whatever the draw)
                nxt = col[e0 + (k == 1 ? 0 : (int64_t)threshold(uniform53(seed, stream, (uint32_t)s, w, (uint32_t)h), (uint64_t)k))];
            } else {
                exhausted = true;
                for (int r = 0; r < PT_TRIALS; ++r) {
                    const uint32_t hop_c = r == 0 ? (uint32_t)h : 0x80000000u + 256u * (uint32_t)r + (uint32_t)h;
                    const int32_t x = col[e0 + (int64_t)threshold(uniform53(seed, stream, (uint32_t)s, w, hop_c), (uint64_t)k)];
                    const uint32_t c = pt_class_of(x, prev, sadj, pe0, pk, bias);
                    bool take = c == bias.w_max;
                    if (!take) {
                        const uint32_t hop_a = 0x40000000u + 256u * (uint32_t)r + (uint32_t)h;
                        take = threshold(uniform53(seed, stream, (uint32_t)s, w, hop_a), (uint64_t)bias.w_max) < (uint64_t)c;
                    }
                    if (take) {
                        nxt = x;
                        exhausted = false;
                        break;
                    }
                }
            }
        }
        // the exact draw, wave-cooperative: W = the class weights of the whole list of cur, t = t(W), the first entry whose
        // inclusive prefix sum exceeds t
        for (uint64_t todo = __ballot(exhausted); todo != 0ull; todo &= todo - 1) {
            const int src = __ffsll((unsigned long long)todo) - 1;
            const int64_t b_e0 = __shfl(e0, src, 64), b_pe0 = __shfl(pe0, src, 64);
            const int32_t b_k = __shfl(k, src, 64), b_pk = __shfl(pk, src, 64), b_prev = __shfl(prev, src, 64);
            const uint32_t b_s = (uint32_t)__shfl(s, src, 64), b_w = (uint32_t)__shfl((int)w, src, 64);
            uint64_t W = 0;
            for (int32_t base = 0; base < b_k; base += 64) {
                const int32_t i = base + lane;
                if (i < b_k) W += pt_class_of(col[b_e0 + i], b_prev, sadj, b_pe0, b_pk, bias);
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) W += (uint64_t)__shfl_xor((long long)W, off, 64);
            const uint32_t hop_f = 0x80000000u + 256u * (uint32_t)PT_TRIALS + (uint32_t)h;
            const uint64_t t = threshold(uniform53(seed, stream, b_s, b_w, hop_f), W);  // (every lane: the same words, no divergence)
            uint64_t run = 0;
            int32_t pick = -1;
            for (int32_t base = 0; base < b_k; base += 64) {
                const int32_t i = base + lane;
                const int32_t x = i < b_k ? col[b_e0 + i] : -1;
                const uint32_t c = i < b_k ? pt_class_of(x, b_prev, sadj, b_pe0, b_pk, bias) : 0u;
                uint32_t inc = c;  // (at most 64 * 65536: 32 bits hold a chunk)
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t y = (uint32_t)__shfl_up((int)inc, off, 64);
                    if (lane >= off) inc += y;
                }
                const uint64_t hit = __ballot(i < b_k && run + inc > t);
                if (hit != 0ull) {
                    pick = __shfl(x, __ffsll((unsigned long long)hit) - 1, 64);
                    break;
                }
                run += (uint64_t)(uint32_t)__shfl((int)inc, 63, 64);
            }
            if (lane == src) nxt = pick;  // (t < W: a hit is certain)
        }
        if (alive) {
            prev = cur;
            pe0 = e0;
            pk = k;
            cur = nxt;
            p[h] = cur;
            len = h + 1;
        }
    }
    if (valid) {
        for (int h = len; h < walk_len; ++h) p[h] = -1;
        path_len[g] = len;
    }
}

// P5: rows of a walk = (1 + n_neg) * pairs of its path
__global__ __launch_bounds__(256) void pt_count_kernel(const int32_t *__restrict__ path_len, int64_t n_walks, int window, int n_neg,
                                                       int32_t *__restrict__ cnt) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_walks) return;
    const int len = path_len[g];
    int c = 0;
    for (int i = 0; i < len; ++i) c += pt_pairs_of(i, len, window);
    cnt[g] = c * (1 + n_neg);
}

// P3-P5.  One wavefront per walk, PT_WAVES walks per workgroup and round; the workgroups stride over the walks so that the
// subsample of the prefix sums is loaded into LDS once per workgroup.  cum == NULL: uniform noise.
//   sample[k] = cum[min((k + 1) * sample_stride, n_node) - 1], k < n_sample <= PT_SAMPLE: the first k with sample[k] > t names
//   the block [k * sample_stride, ...) of cum that holds the first j with cum[j] > t -- the search P4 defines, its first
//   levels taken from LDS.
__global__ __launch_bounds__(256) void pt_fill_kernel(const int32_t *__restrict__ paths, const int32_t *__restrict__ path_len,
                                                      const int32_t *__restrict__ starts, const int64_t *__restrict__ row_ptr,
                                                      int64_t n_walks, int wps, int walk_len, int window, int n_neg, uint64_t seed,
                                                      uint32_t stream, int32_t n_node, const uint64_t *__restrict__ cum,
                                                      uint64_t cum_total, const uint64_t *__restrict__ sample, int n_sample,
                                                      int sample_stride, int32_t *__restrict__ center, int32_t *__restrict__ neighbor,
                                                      float *__restrict__ label) {
    __shared__ uint64_t s_sample[PT_SAMPLE];
    __shared__ int32_t s_path[PT_WAVES][PT_MAX_LEN];
    __shared__ int32_t s_pre[PT_WAVES][PT_MAX_LEN + 4];  // pairs of the centres before i
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (cum)
        for (int i = threadIdx.x; i < n_sample; i += blockDim.x) s_sample[i] = sample[i];
    const int np1 = n_neg + 1;
    // every wavefront of the workgroup runs the same number of rounds (the barriers below are workgroup barriers)
    for (int64_t g0 = (int64_t)blockIdx.x * PT_WAVES; g0 < n_walks; g0 += (int64_t)gridDim.x * PT_WAVES) {
        const int64_t g = g0 + wv;
        const bool valid = g < n_walks;
        const int len = valid ? path_len[g] : 0;
        const int64_t o = valid ? row_ptr[g] : 0;
        const int rows = valid ? (int)(row_ptr[g + 1] - o) : 0;
        int run = 0;
        if (rows > 0) {
            for (int base = 0; base < len; base += 64) {
                const int i = base + lane;
                const int c = i < len ? pt_pairs_of(i, len, window) : 0;
                if (i < len) s_path[wv][i] = paths[g * walk_len + i];
                int inc = c;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int x = __shfl_up(inc, off, 64);
                    if (lane >= off) inc += x;
                }
                if (i < len) s_pre[wv][i] = run + inc - c;
                run += __shfl(inc, 63, 64);
            }
        }
        __syncthreads();
        if (rows > 0) {
            const int64_t si = g / wps;
            const uint32_t w = (uint32_t)(g - si * wps);
            const uint32_t root = (uint32_t)starts[si];
            for (int r = lane; r < rows; r += 64) {
                const int p = r / np1, q = r - p * np1;
                // centre i: the last one with s_pre[i] <= p (len >= 2 here, so every centre has a pair and s_pre is strictly increasing)
                int lo = 0, hi = len - 1;
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (s_pre[wv][mid] <= p) lo = mid;
                    else hi = mid - 1;
                }
                const int i = lo;
                int j = max(i - window, 0) + (p - s_pre[wv][i]);
                if (j >= i) ++j;
                const int32_t c = s_path[wv][i], x = s_path[wv][j];
                int32_t nb = x;
                float lab = 1.0f;
                if (q > 0) {
                    const uint64_t m = uniform53(seed, stream, root, w, (uint32_t)(walk_len + p * n_neg + (q - 1)));
                    int32_t node;
                    if (cum) {
                        const uint64_t t = threshold(m, cum_total);
                        int a = 0, b = n_sample - 1;  // sample[n_sample - 1] = cum_total > t
                        while (a < b) {
                            const int mid = (a + b) >> 1;
                            if (s_sample[mid] > t) b = mid;
                            else a = mid + 1;
                        }
                        int32_t l2 = a * sample_stride, h2 = min(l2 + sample_stride, n_node) - 1;  // cum[h2] = sample[a] > t, cum[l2 - 1] <= t
                        while (l2 < h2) {
                            const int32_t mid = l2 + ((h2 - l2) >> 1);
                            if (cum[mid] > t) h2 = mid;
                            else l2 = mid + 1;
                        }
                        node = l2;
                    } else {
                        node = (int32_t)threshold(m, (uint64_t)n_node);
                    }
                    while (node == c || node == x) node = node + 1 == n_node ? 0 : node + 1;  // at most two steps (n_node >= 3)
                    nb = node;
                    lab = 0.0f;
                }
                center[o + r] = c;
                neighbor[o + r] = nb;
                label[o + r] = lab;
            }
        }
        __syncthreads();  // the next round overwrites s_path / s_pre
    }
}

}  // namespace gg

using namespace gg;

extern "C" {

int gg_pretrain_set_noise(gg_ctx *ctx, const uint32_t *weight) {
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    GG_HIP(ctx, hipSetDevice(ctx->device));
    GG_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (a fill kernel of an earlier call may still read the table)
    if (!weight) {
        ctx->pt_noise_set = false;
        return GG_OK;
    }
    const int64_t n = ctx->n_node;
    std::vector<uint64_t> cum((size_t)n);
    uint64_t run = 0;
    for (int64_t j = 0; j < n; ++j) cum[j] = (run += weight[j]);
    GG_CHECK(ctx, run >= 1, GG_EINVAL, "gg_pretrain_set_noise: every weight is zero");
    const int64_t stride = (n + PT_SAMPLE - 1) / PT_SAMPLE, ns = (n + stride - 1) / stride;
    std::vector<uint64_t> sample((size_t)ns);
    for (int64_t k = 0; k < ns; ++k) sample[k] = cum[std::min<int64_t>((k + 1) * stride, n) - 1];
    ctx->pt_noise_set = false;
    GG_HIP(ctx, ctx->pt_noise.reserve(sizeof(uint64_t) * (size_t)n));
    GG_HIP(ctx, ctx->pt_sample.reserve(sizeof(uint64_t) * PT_SAMPLE));
    GG_HIP(ctx, hipMemcpy(ctx->pt_noise.p, cum.data(), sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice));
    GG_HIP(ctx, hipMemcpy(ctx->pt_sample.p, sample.data(), sizeof(uint64_t) * (size_t)ns, hipMemcpyHostToDevice));
    ctx->pt_noise_total = run;
    ctx->pt_sample_n = (int32_t)ns;
    ctx->pt_sample_stride = (int32_t)stride;
    ctx->pt_noise_set = true;
    return GG_OK;
}

int gg_pretrain_set_walk_bias(gg_ctx *ctx, uint32_t w_ret, uint32_t w_com, uint32_t w_out) {
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    for (uint32_t v : {w_ret, w_com, w_out})
        GG_CHECK(ctx, v >= 1 && v <= 65536, GG_EINVAL, "gg_pretrain_set_walk_bias: weights must be in [1, 65536], got (%u, %u, %u)", w_ret, w_com, w_out);
    ctx->pt_bias[0] = w_ret;
    ctx->pt_bias[1] = w_com;
    ctx->pt_bias[2] = w_out;
    return GG_OK;
}

int gg_prepare_pretrain(gg_ctx *ctx, const int32_t *starts, int32_t n_starts, int32_t walks_per_start, int32_t walk_len,
                        int32_t window, int32_t n_neg, uint64_t seed, uint32_t stream, int64_t *n_rows_out, int32_t *paths,
                        int32_t *path_len) {
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    GG_CHECK(ctx, ctx->g_rowptr, GG_EINVAL, "gg_prepare_pretrain: call gg_set_graph_csr first");
    GG_CHECK(ctx, !ctx->comm, GG_EINVAL, "gg_prepare_pretrain: a communicator is attached (pre-training is single rank)");
    GG_CHECK(ctx, !ctx->ep_d_open, GG_EINVAL, "gg_prepare_pretrain: called between gg_epoch_begin and gg_epoch_commit(1)");
    GG_CHECK(ctx, n_starts >= 0 && (starts || n_starts == 0), GG_EINVAL, "gg_prepare_pretrain: bad starts");
    GG_CHECK(ctx, walks_per_start >= 1, GG_EINVAL, "gg_prepare_pretrain: walks_per_start must be >= 1");
    GG_CHECK(ctx, walk_len >= 1 && walk_len <= PT_MAX_LEN, GG_EINVAL, "gg_prepare_pretrain: walk_len must be in [1, %d]", PT_MAX_LEN);
    GG_CHECK(ctx, window >= 1 && window <= PT_MAX_WINDOW, GG_EINVAL, "gg_prepare_pretrain: window must be in [1, %d]", PT_MAX_WINDOW);
    GG_CHECK(ctx, n_neg >= 0 && n_neg <= PT_MAX_NEG, GG_EINVAL, "gg_prepare_pretrain: n_neg must be in [0, %d]", PT_MAX_NEG);
    GG_CHECK(ctx, ctx->n_node >= 3, GG_EINVAL, "gg_prepare_pretrain: the collision rule of the negatives needs n_node >= 3");
    for (int32_t i = 0; i < n_starts; ++i)
        GG_CHECK(ctx, starts[i] >= 0 && starts[i] < ctx->n_node, GG_EINVAL, "gg_prepare_pretrain: starts[%d] = %d out of range", i, starts[i]);
    const int64_t nw = (int64_t)n_starts * walks_per_start;
    GG_CHECK(ctx, nw <= 0x7fffffffll, GG_ECAPACITY, "gg_prepare_pretrain: %lld walks in one call", (long long)nw);
    GG_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t *wb = ctx->pt_bias;
    const bool biased = !(wb[0] == wb[1] && wb[1] == wb[2]);  // equal weights are P2 itself: the uniform kernel, untouched
    if (biased && nw > 0) {
        const int rc = ensure_sorted_adjacency(ctx);
        if (rc != GG_OK) return rc;
    }
    ctx->d_rows = 0;
    if (nw > 0) {
        // rows of a walk that reaches its full length: the capacity rule of the row buffers
        const int64_t rows_bound = nw * (1 + n_neg) * pt_pairs_of_path(walk_len, window);
        const bool sized = rows_bound <= 0x7fffffffll;  // else: the exact total decides (one more synchronisation)
        GG_HIP(ctx, ctx->pt_starts.reserve(sizeof(int32_t) * (size_t)n_starts));
        GG_HIP(ctx, ctx->pt_paths.reserve(sizeof(int32_t) * (size_t)nw * walk_len));
        GG_HIP(ctx, ctx->pt_len.reserve(sizeof(int32_t) * (size_t)nw));
        GG_HIP(ctx, ctx->pt_cnt.reserve(sizeof(int32_t) * (size_t)nw));
        GG_HIP(ctx, ctx->pt_ptr.reserve(sizeof(int64_t) * (size_t)(nw + 1)));
        const bool timed = ctx->profile_every == 1;
        if (timed && !ctx->pt_ev[0])
            for (hipEvent_t &e : ctx->pt_ev) GG_HIP(ctx, hipEventCreate(&e));
        GG_HIP(ctx, hipMemcpyAsync(ctx->pt_starts.p, starts, sizeof(int32_t) * (size_t)n_starts, hipMemcpyHostToDevice, ctx->stream));
        if (timed) GG_HIP(ctx, hipEventRecord(ctx->pt_ev[0], ctx->stream));
        if (biased)
            hipLaunchKernelGGL(pt_walk_bias_kernel, dim3(cdiv(nw, 256)), dim3(256), 0, ctx->stream, ctx->g_rowptr, ctx->g_col,
                               ctx->topk_adj.as<int32_t>(), ctx->pt_starts.as<int32_t>(), nw, walks_per_start, walk_len, seed, stream,
                               PtBias{wb[0], wb[1], wb[2], std::max(wb[0], std::max(wb[1], wb[2]))}, ctx->pt_paths.as<int32_t>(),
                               ctx->pt_len.as<int32_t>());
        else
            hipLaunchKernelGGL(pt_walk_kernel, dim3(cdiv(nw, 256)), dim3(256), 0, ctx->stream, ctx->g_rowptr, ctx->g_col,
                               ctx->pt_starts.as<int32_t>(), nw, walks_per_start, walk_len, seed, stream, ctx->pt_paths.as<int32_t>(),
                               ctx->pt_len.as<int32_t>());
        if (timed) GG_HIP(ctx, hipEventRecord(ctx->pt_ev[1], ctx->stream));
        hipLaunchKernelGGL(pt_count_kernel, dim3(cdiv(nw, 256)), dim3(256), 0, ctx->stream, ctx->pt_len.as<int32_t>(), nw, window, n_neg,
                           ctx->pt_cnt.as<int32_t>());
        GG_HIP(ctx, hipGetLastError());
        int rc = device_exclusive_scan(ctx, ctx->pt_cnt.as<int32_t>(), ctx->pt_ptr.as<int64_t>(), nw);
        if (rc != GG_OK) return rc;
        GG_HIP(ctx, hipMemcpyAsync(ctx->h_pin + H_PT_TOTAL, ctx->pt_ptr.as<int64_t>() + nw, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        int64_t cap = rows_bound;
        if (!sized) {
            GG_HIP(ctx, hipStreamSynchronize(ctx->stream));
            cap = (int64_t)ctx->h_pin[H_PT_TOTAL];
            GG_CHECK(ctx, cap <= 0x7fffffffll, GG_ECAPACITY, "gg_prepare_pretrain: %lld rows in one call (at most 2^31 - 1): pass fewer starts",
                     (long long)cap);
        }
        GG_HIP(ctx, ctx->d_center.reserve(sizeof(int32_t) * (size_t)(cap + 1)));
        GG_HIP(ctx, ctx->d_neighbor.reserve(sizeof(int32_t) * (size_t)(cap + 1)));
        GG_HIP(ctx, ctx->d_label.reserve(sizeof(float) * (size_t)(cap + 1)));
        const bool noise = ctx->pt_noise_set;
        const int64_t blocks = std::min<int64_t>((nw + PT_WAVES - 1) / PT_WAVES, (int64_t)ctx->n_cus * 12);
        if (timed) GG_HIP(ctx, hipEventRecord(ctx->pt_ev[2], ctx->stream));
        hipLaunchKernelGGL(pt_fill_kernel, dim3((unsigned)blocks), dim3(64 * PT_WAVES), 0, ctx->stream, ctx->pt_paths.as<int32_t>(),
                           ctx->pt_len.as<int32_t>(), ctx->pt_starts.as<int32_t>(), ctx->pt_ptr.as<int64_t>(), nw, walks_per_start, walk_len,
                           window, n_neg, seed, stream, ctx->n_node, noise ? ctx->pt_noise.as<uint64_t>() : (const uint64_t *)nullptr,
                           noise ? ctx->pt_noise_total : 0ull, ctx->pt_sample.as<uint64_t>(), noise ? ctx->pt_sample_n : 0,
                           noise ? ctx->pt_sample_stride : 1, ctx->d_center.as<int32_t>(), ctx->d_neighbor.as<int32_t>(),
                           ctx->d_label.as<float>());
        if (timed) GG_HIP(ctx, hipEventRecord(ctx->pt_ev[3], ctx->stream));
        GG_HIP(ctx, hipGetLastError());
        GG_HIP(ctx, hipStreamSynchronize(ctx->stream));
        harvest_timings(ctx);
        ctx->d_rows = (int64_t)ctx->h_pin[H_PT_TOTAL];
        if (timed) {
            float walk_ms = 0.f, fill_ms = 0.f;
            GG_HIP(ctx, hipEventElapsedTime(&walk_ms, ctx->pt_ev[0], ctx->pt_ev[1]));
            GG_HIP(ctx, hipEventElapsedTime(&fill_ms, ctx->pt_ev[2], ctx->pt_ev[3]));
            ctx->ctr.walk_kernel_ms += walk_ms;  // (the walk launch of this prepare call; the tree walks' figures are per call site)
            ctx->ctr.walk_launches += 1;
            ctx->ctr.last_kernel_ms = fill_ms;
        }
        if (paths) GG_HIP(ctx, hipMemcpy(paths, ctx->pt_paths.p, sizeof(int32_t) * (size_t)nw * walk_len, hipMemcpyDeviceToHost));
        if (path_len) GG_HIP(ctx, hipMemcpy(path_len, ctx->pt_len.p, sizeof(int32_t) * (size_t)nw, hipMemcpyDeviceToHost));
    } else {
        GG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    ctx->d_rows_max = ctx->d_rows;  // (single rank: no replica exchange of the count)
    if (n_rows_out) *n_rows_out = ctx->d_rows;
    return GG_OK;
}

}  // extern "C"
