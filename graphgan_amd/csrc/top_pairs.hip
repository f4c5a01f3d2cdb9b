// top_pairs.hip -- global top-K pair prediction: the k best-scored unordered pairs {u, v}, u < v, of a node set under
// s(u, v) = E[u] . E[v] (no bias), optionally without the pairs whose v is a neighbour of u in the resident training graph.  The
// fourth consumer of the tile stream (score_tiles.h), with u as the row and v as the column, and as cheap per tile as the rank
// consumer: every score of every row is compared with ONE global floor.  Nothing of size rows x columns exists at any time.
//
// Order: (s, u, v) is ahead of (s', u', v') when ord(s) > ord(s') (ord of topk_score.hip's key: -0 counts as +0), or the ords are
// equal and (u, v) < (u', v') lexicographically; on finite scores that is
//     s > s'  ||  (s == s'  &&  (u < u'  ||  (u == u'  &&  v < v')))
// in fp32 and integer compares, which is what the kernels evaluate.
//
// Device side.  A floor triple (fs, fu, fv) sits in device memory: the k-th best pair found so far, (-inf, max, max) until k pairs
// are known.  A kernel reads it once.  Per tile and lane the 16 scores are compared with fs (>=) and OR-ed into one ballot; the
// rare tiles with a hit take the slow path: per score the full triple compare (strictly ahead of the floor), column id > row id,
// the membership bit of the column (instances with a `nodes` bitmap), the binary search in the sorted adjacency (exclude), and
// then an append of (score bits, u, v) to a global buffer -- ONE integer atomic per wavefront and tile on the fill counter.  The
// counter keeps counting past the capacity, the stores do not.
//
// Host schedule (PairRun).  A launch is a rectangle: a range of 32-row tiles x a column range in multiples of 128; every
// row tile starts its sweep at the 128-column tile that holds its smallest row id, tiles wholly at or below the diagonal are not
// computed.  One 4-byte read-back of the fill counter per launch.  Overflow: the counter is set back to its value before the
// launch, the buffer is compacted if it holds more than k entries, and the rectangle is rerun as two halves (rows first, then
// columns); one 32 x 128 tile always fits behind k entries, hence buffer_entries >= k + 4096.  The first rectangle holds at most
// buffer_entries - k pairs, later ones double up to 4 096 rows x all columns (and 2^32 - 2^27 pairs: the counter has 32 bits).  A
// compaction (fill above PairRun::compact_above(), and at the end) selects the k best entries on the host (sorted at the end only)
// and stores the k-th as the new floor.  The floor only ever drops pairs that k known pairs are ahead of, so the result is exact
// and a function of the table, the set and the graph alone -- not of the buffer, the rectangles or the order of the appends.
#include <math.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "score_tiles.h"

namespace gg {

namespace {

constexpr int64_t TP_MAX_K = 1 << 20;
constexpr int64_t TP_MIN_BUF = 1 << 22, TP_MAX_BUF = 1 << 26;
constexpr int64_t TP_TILE = 32 * 128;           // pairs of the smallest rectangle
constexpr int TP_MAX_ROW_TILES = 4096 / 32;     // row tiles of the largest rectangle
constexpr int64_t TP_MAX_AREA = (int64_t(1) << 32) - (int64_t(1) << 27);  // pairs of the largest rectangle: with the 2^26 entries a buffer
                                                                          // holds at most, the 32-bit fill counter cannot wrap

struct PairArgs {
    const int32_t *nodes;     // [m] the set, ascending (NULL: node r is row r, m = n_node)
    int m;
    const uint32_t *member;   // [ceil(n_node / 32)] bit c: column c is in the set (instances with a bitmap)
    const int64_t *adj_ptr;   // exclusion: the graph's row offsets and its column lists sorted per node (NULL: exclude = 0)
    const int32_t *adj;
    const uint32_t *floor;    // [3] fs (fp32 bits), fu, fv
    uint32_t *fill;           // entries appended so far (counts on past cap)
    uint32_t cap;
    uint4 *buf;               // [cap] (score bits, u, v, 0)
    int rt0;                  // the rectangle: first row tile, columns [cbeg, cend), cbeg a multiple of 128, split in parts of
    int cbeg, cend, cps;      // cps columns (a multiple of 128) over blockIdx.x
};

__device__ __forceinline__ bool tp_adj_contains(const int32_t *a, int64_t n, int col) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < col) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && a[lo] == col;
}

// The consumer handed to the producers of score_tiles.h.  BM: the rows are o.nodes[r0 ..] and a column must have its bit in
// o.member; without, row r is node r and every column is in the set.
template <bool BM>
struct FloorConsumer {
    float fs;
    int fu, fv;
    const PairArgs &o;
    const int r0;
    __device__ __forceinline__ FloorConsumer(const PairArgs &o_, int r0_) : o(o_), r0(r0_) {}
    __device__ __forceinline__ void init() {
        fs = __uint_as_float(o.floor[0]);
        fu = (int)o.floor[1];
        fv = (int)o.floor[2];
    }
    __device__ __forceinline__ float start(int, bool) const { return 0.f; }
    __device__ __forceinline__ float pick(const f32x16 &acc, int reg) const {
        float x = acc[0];
#pragma unroll
        for (int r2 = 1; r2 < 16; ++r2) x = reg == r2 ? acc[r2] : x;
        return x;
    }
    __device__ __forceinline__ void operator()(const f32x16 &acc, int col, bool ok) {
        bool any = false;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) any |= acc[reg] >= fs;
        any &= ok;
        if (!__builtin_amdgcn_ballot_w64(any)) return;
        // slow path: which of the lane's 16 scores are candidates ahead of the floor
        const int lane = threadIdx.x & 63, half = lane >> 5;
        uint32_t mask = 0;
#pragma unroll 1
        for (int reg = 0; reg < 16; ++reg) {
            const float x = pick(acc, reg);
            const int row = r0 + tile_row(reg, half);
            if (!(ok && row < o.m && x >= fs)) continue;
            const int u = BM ? o.nodes[row] : row;
            bool p = (x > fs || u < fu || (u == fu && col < fv)) && col > u;
            if (BM && p) p = ((o.member[col >> 5] >> (col & 31)) & 1u) != 0;
            if (p && o.adj) {
                const int64_t b = o.adj_ptr[u], e = o.adj_ptr[u + 1];
                p = !tp_adj_contains(o.adj + b, e - b, col);
            }
            mask |= (p ? 1u : 0u) << reg;
        }
        // one slot range per wavefront: inclusive scan of the lanes' counts, one atomic by lane 0
        const int cnt = __builtin_popcount(mask);
        int incl = cnt;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off, 64);
            incl += lane >= off ? t : 0;
        }
        const int total = __shfl(incl, 63, 64);
        if (total == 0) return;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(o.fill, (uint32_t)total);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        uint32_t at = base + (uint32_t)(incl - cnt);
#pragma unroll 1
        for (int reg = 0; reg < 16; ++reg) {
            if (!((mask >> reg) & 1u)) continue;
            const float x = pick(acc, reg);
            const int row = r0 + tile_row(reg, half);
            const int u = BM ? o.nodes[row] : row;
            if (at < o.cap) o.buf[at] = make_uint4(__float_as_uint(x), (uint32_t)u, (uint32_t)col, 0u);
            ++at;
        }
    }
    __device__ __forceinline__ void operator()(const f32x16 (&acc)[1], int col, bool ok) { (*this)(acc[0], col, ok); }
};

// The workgroup's column range [c0, c1) of its row tile: its part of the rectangle's columns, from the 128-column tile that
// holds the tile's smallest row id.  Workgroup-uniform.
template <bool BM>
__device__ __forceinline__ bool tp_range(const PairArgs &o, int n_node, int r0, int &c0, int &c1) {
    if (r0 >= o.m) return false;
    const int first = BM ? o.nodes[r0] : r0;
    c0 = o.cbeg + (int)blockIdx.x * o.cps;
    c1 = min(min(o.cend, n_node), c0 + o.cps);
    c0 = max(c0, first & ~127);
    return c0 < c1;
}

// grid = (column parts, row tiles of the rectangle), 4 wavefronts of 32 columns each.
template <bool BM>
__global__ __launch_bounds__(256) void tp_f32_kernel(const float *E, int n_node, int ld, PairArgs o) {
    extern __shared__ float As_all[];  // [32][ld + 1]: the tile's 32 rows, staged once
    __shared__ float Bs[128][ST_KC + 1];
    const int r0 = (o.rt0 + (int)blockIdx.y) * 32;
    int c0, c1;
    if (!tp_range<BM>(o, n_node, r0, c0, c1)) return;
    FloorConsumer<BM> pairs(o, r0);
    f32_score_tiles(E, ld, o.nodes, o.m, r0, c0, c1, As_all, Bs, pairs);
}

template <int KS, bool BM>
__global__ __launch_bounds__(256) void tp_bf16_kernel(const uint4 *Eb, int n_node, PairArgs o) {
    const int r0 = (o.rt0 + (int)blockIdx.y) * 32;
    int c0, c1;
    if (!tp_range<BM>(o, n_node, r0, c0, c1)) return;
    FloorConsumer<BM> pairs(o, r0);
    bf16_score_tiles<KS, 1, (KS <= 16)>(Eb, o.nodes, o.m, r0, c0, c1, pairs);
}

template <bool BM>
void tp_launch(gg_ctx *ctx, const Model &M, int precision, int KS, const uint4 *Eb, size_t dyn, dim3 grid, const PairArgs &o) {
    const int n = ctx->n_node;
    if (precision == 0) hipLaunchKernelGGL(tp_f32_kernel<BM>, grid, dim3(256), dyn, ctx->stream, M.E, n, ctx->ld, o);
    else if (KS == 4) hipLaunchKernelGGL((tp_bf16_kernel<4, BM>), grid, dim3(256), 0, ctx->stream, Eb, n, o);
    else if (KS == 8) hipLaunchKernelGGL((tp_bf16_kernel<8, BM>), grid, dim3(256), 0, ctx->stream, Eb, n, o);
    else if (KS == 16) hipLaunchKernelGGL((tp_bf16_kernel<16, BM>), grid, dim3(256), 0, ctx->stream, Eb, n, o);
    else hipLaunchKernelGGL((tp_bf16_kernel<32, BM>), grid, dim3(256), 0, ctx->stream, Eb, n, o);
}

// the monotone unsigned image of an fp32 (topk_score.hip's ord: -0 counts as +0)
inline uint32_t tp_ord(uint32_t u) {
    u = u == 0x80000000u ? 0u : u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct Entry {
    uint32_t s, u, v, pad;
};
inline bool entry_ahead(const Entry &a, const Entry &b) {
    const uint32_t oa = tp_ord(a.s), ob = tp_ord(b.s);
    if (oa != ob) return oa > ob;
    if (a.u != b.u) return a.u < b.u;
    return a.v < b.v;
}

struct Rect {
    int rt0, rt1, cbeg, cend;  // row tiles [rt0, rt1), columns [cbeg, cend)
};

// The whole run behind the checks.
struct PairRun {
    gg_ctx *ctx;
    const Model *M;
    int precision, KS;
    bool bitmap;
    size_t dyn;
    const uint4 *Eb;
    PairArgs o;
    int64_t k, cap;
    const int32_t *h_nodes;  // host copy of the set (NULL: all nodes)
    uint32_t *d_floor;
    int64_t fill = 0;        // the device counter, as the host knows it
    int64_t launches = 0, retries = 0, compactions = 0, appended = 0;
    double compact_s = 0.0;
    std::vector<Entry> h;
    hipError_t e = hipSuccess;
    bool internal = false;   // a single tile did not fit: cannot happen

    int first_col(int rt) const { return (h_nodes ? h_nodes[(int64_t)rt * 32] : rt * 32) & ~127; }

    // fill above this: compact.  About e k entries keep the host's work over a whole sweep smallest (a compaction costs its
    // entries, and the pairs seen grow by the factor 1 + (entries - k) / k between two of them); at least 2^16, so that a small k
    // does not compact after every launch, and the middle between k and the capacity at most.
    int64_t compact_above() const { return std::min(k + (cap - k) / 2, std::max<int64_t>(3 * k, int64_t(1) << 16)); }

    // the fill entries of the buffer to the host, the k best kept and written back, the k-th as the new floor; sorted only at the end
    void compact(bool last = false) {
        const auto t0 = std::chrono::steady_clock::now();
        h.resize((size_t)fill);
        if (fill) e = hipMemcpyAsync(h.data(), o.buf, sizeof(Entry) * (size_t)fill, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return;
        const size_t keep = (size_t)std::min<int64_t>(fill, k);
        if (keep) std::nth_element(h.begin(), h.begin() + (keep - 1), h.end(), entry_ahead);  // the keep-th best at keep - 1, the better ones in front
        h.resize(keep);
        uint32_t head[4] = {0xff800000u, 0x7fffffffu, 0x7fffffffu, (uint32_t)keep};  // floor (below everything), then the counter
        if ((int64_t)keep == k) { head[0] = h[keep - 1].s; head[1] = h[keep - 1].u; head[2] = h[keep - 1].v; }
        if (last) {
            std::sort(h.begin(), h.end(), entry_ahead);
            ++compactions;
            compact_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            return;
        }
        if (keep) e = hipMemcpyAsync(o.buf, h.data(), sizeof(Entry) * keep, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_floor, head, sizeof(head), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        fill = (int64_t)keep;
        ++compactions;
        compact_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }

    void run(const Rect &r) {
        if (e != hipSuccess || internal) return;
        const int nt = r.rt1 - r.rt0;
        const int c_lo = std::max(r.cbeg, first_col(r.rt0));
        if (nt <= 0 || c_lo >= r.cend) return;
        const int tiles = cdiv(r.cend - c_lo, 128);
        const int parts = std::max(1, std::min(tiles, 2048 / nt));
        PairArgs a = o;
        a.rt0 = r.rt0;
        a.cbeg = c_lo;
        a.cend = r.cend;
        a.cps = cdiv(tiles, parts) * 128;
        const dim3 grid(cdiv(tiles * 128, a.cps), nt);
        if (bitmap) tp_launch<true>(ctx, *M, precision, KS, Eb, dyn, grid, a);
        else tp_launch<false>(ctx, *M, precision, KS, Eb, dyn, grid, a);
        ++launches;
        e = hipGetLastError();
        uint32_t now = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&now, o.fill, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return;
        if ((int64_t)now <= cap) {
            appended += (int64_t)now - fill;
            fill = now;
            if (fill > compact_above()) compact();
            return;
        }
        // overflow: the counter back to its value before the launch, then the halves
        ++retries;
        const uint32_t before = (uint32_t)fill;
        e = hipMemcpyAsync(o.fill, &before, sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return;
        if (fill > k) compact();
        if (nt > 1) {
            const int mid = r.rt0 + nt / 2;
            run(Rect{r.rt0, mid, r.cbeg, r.cend});
            run(Rect{mid, r.rt1, r.cbeg, r.cend});
        } else if (tiles > 1) {
            const int mid = c_lo + (tiles / 2) * 128;
            run(Rect{r.rt0, r.rt1, c_lo, mid});
            run(Rect{r.rt0, r.rt1, mid, r.cend});
        } else {
            internal = true;
        }
    }

    // every rectangle of the triangle: the first holds at most cap - k pairs, the budget doubles per launch
    void sweep(int n_node) {
        const int T = cdiv(o.m, 32);
        const int n_up = cdiv(n_node, 128) * 128;
        int64_t area = std::max<int64_t>(cap - k, TP_TILE);
        int rt = 0, c = -1;  // c: the column cursor inside a row tile that is swept in several rectangles (-1: at its start)
        while (rt < T && e == hipSuccess && !internal) {
            const int cs = c < 0 ? first_col(rt) : c;
            const int64_t w = n_up - cs;
            if (w <= 0) { ++rt; c = -1; continue; }
            if (c < 0 && 32 * w <= area) {
                const int nt = (int)std::min<int64_t>(std::min(T - rt, TP_MAX_ROW_TILES), area / (32 * w));
                run(Rect{rt, rt + nt, cs, n_node});
                rt += nt;
            } else {
                const int64_t cw = std::max<int64_t>(128, area / 32 / 128 * 128);
                const int ce = (int)std::min<int64_t>(n_up, cs + cw);
                run(Rect{rt, rt + 1, cs, std::min(ce, n_node)});
                c = ce;
                if (c >= n_node) { ++rt; c = -1; }
            }
            area = std::min(area * 2, TP_MAX_AREA);
        }
    }
};

}  // namespace

}  // namespace gg

using namespace gg;

// gg_top_pairs: see include/graphgan_hip.h.
extern "C" int gg_top_pairs(gg_ctx *ctx, int32_t which, int32_t precision, const int32_t *nodes, int64_t m, int64_t k, int32_t exclude,
                            int64_t buffer_entries, int32_t *u_out, int32_t *v_out, float *score_out, int64_t *n_found, int64_t *stats, double *ms_out) {
    const char *fn = "gg_top_pairs";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    GG_CHECK(ctx, which == 0 || which == 1, GG_EINVAL, "%s: which must be 0 (generator) or 1 (discriminator)", fn);
    GG_CHECK(ctx, precision == 0 || precision == 1, GG_EINVAL, "%s: precision must be 0 (fp32) or 1 (bf16)", fn);
    GG_CHECK(ctx, exclude == 0 || exclude == 1, GG_EINVAL, "%s: exclude must be 0 or 1", fn);
    GG_CHECK(ctx, k >= 1 && k <= TP_MAX_K, GG_EINVAL, "%s: k = %lld outside [1, 2^20]", fn, (long long)k);
    GG_CHECK(ctx, u_out && v_out && score_out && n_found && (!nodes || m >= 0), GG_EINVAL, "%s: bad argument", fn);
    GG_CHECK(ctx, buffer_entries == 0 || (buffer_entries >= k + TP_TILE && buffer_entries <= TP_MAX_BUF), GG_EINVAL,
             "%s: buffer_entries = %lld outside [k + 4096, 2^26] (0: the default)", fn, (long long)buffer_entries);
    GG_CHECK(ctx, !exclude || ctx->g_rowptr, GG_EINVAL, "%s: exclude = 1 needs the training graph (gg_set_graph_csr)", fn);
    const int n = ctx->n_node, ld = ctx->ld;
    GG_CHECK(ctx, precision == 0 || ctx->n_emb <= 512, GG_EINVAL, "%s: bf16 supports n_emb <= 512 (got %d)", fn, ctx->n_emb);
    const size_t dyn = sizeof(float) * 32 * (size_t)(ld + 1);
    GG_CHECK(ctx, precision == 1 || dyn <= 140 * 1024, GG_EINVAL, "%s: fp32 supports n_emb <= 1116 (got %d)", fn, ctx->n_emb);
    if (nodes)
        for (int64_t i = 0; i < m; ++i) {
            GG_CHECK(ctx, nodes[i] >= 0 && nodes[i] < n, GG_EINVAL, "%s: nodes[%lld] = %d out of range [0, %d)", fn, (long long)i, nodes[i], n);
            GG_CHECK(ctx, i == 0 || nodes[i] > nodes[i - 1], GG_EINVAL, "%s: nodes[%lld] = %d is not above nodes[%lld] = %d (strictly ascending ids)", fn,
                     (long long)i, nodes[i], (long long)(i - 1), nodes[i - 1]);
        }
    if (!nodes) m = n;
    for (int64_t i = 0; i < k; ++i) { u_out[i] = -1; v_out[i] = -1; score_out[i] = -INFINITY; }
    *n_found = 0;
    if (stats) for (int i = 0; i < 6; ++i) stats[i] = 0;
    if (ms_out) *ms_out = 0.0;
    if (m < 2) return GG_OK;
    GG_HIP(ctx, hipSetDevice(ctx->device));
    if (exclude) {
        const int rc = ensure_sorted_adjacency(ctx);
        if (rc != GG_OK) return rc;
    }
    const int64_t cap = buffer_entries ? buffer_entries : std::max<int64_t>(TP_MIN_BUF, 4 * k);
    const Bf16Shape bs = bf16_shape(ctx->n_emb);
    const int n_words = cdiv(n, 32);
    ScopedBuf d_nodes, d_member, d_head, d_buf, d_bf;
    std::vector<uint32_t> member;
    hipError_t e = d_head.reserve(sizeof(uint32_t) * 4);
    if (e == hipSuccess) e = d_buf.reserve(sizeof(Entry) * (size_t)cap);
    if (e == hipSuccess && nodes) e = d_nodes.reserve(sizeof(int32_t) * (size_t)m);
    if (e == hipSuccess && nodes) e = d_member.reserve(sizeof(uint32_t) * (size_t)n_words);
    if (e == hipSuccess && precision == 1) e = bf16_table(ctx, which, bs.ld16, d_bf);
    if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "%s: %s", fn, hipGetErrorString(e));
    if (nodes) {
        member.assign(n_words, 0u);
        for (int64_t i = 0; i < m; ++i) member[nodes[i] >> 5] |= 1u << (nodes[i] & 31);
        e = hipMemcpyAsync(d_nodes.p, nodes, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_member.p, member.data(), sizeof(uint32_t) * (size_t)n_words, hipMemcpyHostToDevice, ctx->stream);
    }
    const uint32_t head[4] = {0xff800000u, 0x7fffffffu, 0x7fffffffu, 0u};  // the floor below everything, the counter at 0
    if (e == hipSuccess) e = hipMemcpyAsync(d_head.p, head, sizeof(head), hipMemcpyHostToDevice, ctx->stream);
    if (precision == 0 && dyn > 48 * 1024) {
        (void)hipFuncSetAttribute((const void *)tp_f32_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
        (void)hipFuncSetAttribute((const void *)tp_f32_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    }
    PairRun R;
    R.ctx = ctx;
    R.M = &ctx->model[which];
    R.precision = precision;
    R.KS = bs.KS;
    R.bitmap = nodes != nullptr;
    R.dyn = dyn;
    R.Eb = (const uint4 *)d_bf.p;
    R.k = k;
    R.cap = cap;
    R.h_nodes = nodes;
    R.d_floor = d_head.as<uint32_t>();
    R.o = PairArgs{d_nodes.as<int32_t>(), (int)m, d_member.as<uint32_t>(), exclude ? ctx->g_rowptr : nullptr, exclude ? ctx->topk_adj.as<int32_t>() : nullptr,
                   d_head.as<uint32_t>(), d_head.as<uint32_t>() + 3, (uint32_t)cap, d_buf.as<uint4>(), 0, 0, 0, 128};
    R.e = e;
    if (e == hipSuccess) (void)hipEventRecord(ctx->ev0, ctx->stream);
    if (e == hipSuccess) R.sweep(n);
    if (R.e == hipSuccess && !R.internal) R.compact(true);  // the k best, sorted, in R.h
    if (R.e == hipSuccess) (void)hipEventRecord(ctx->ev1, ctx->stream);
    if (R.e == hipSuccess) R.e = hipStreamSynchronize(ctx->stream);
    else (void)hipStreamSynchronize(ctx->stream);  // (the set's source and the buffers go away behind it)
    if (R.e != hipSuccess) return fail(ctx, GG_EHIP, "%s: %s", fn, hipGetErrorString(R.e));
    if (R.internal) return fail(ctx, GG_ECAPACITY, "%s: internal error: one 32 x 128 tile overflowed a buffer of %lld entries behind %lld", fn, (long long)cap, (long long)k);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    for (size_t i = 0; i < R.h.size(); ++i) {
        u_out[i] = (int32_t)R.h[i].u;
        v_out[i] = (int32_t)R.h[i].v;
        const uint32_t bits = R.h[i].s;
        std::memcpy(score_out + i, &bits, sizeof(float));
    }
    *n_found = (int64_t)R.h.size();
    if (stats) {
        stats[0] = R.launches;
        stats[1] = R.retries;
        stats[2] = R.compactions;
        stats[3] = R.appended;
        stats[4] = (int64_t)(R.compact_s * 1e6);
        stats[5] = cap;
    }
    if (ms_out) *ms_out = ms;
    return GG_OK;
}
