// two_hop.hip -- the two-hop sweep behind the graph-only ranking baselines: per query u one row of A W A on the resident training
// graph, S(u, c) = sum over w in N(u) & N(c) of weights[w] (unsigned 64-bit integers; no weights: common neighbours), and from
// it either the best k candidates (gg_two_hop_topk) or the integers that place one target in the total order (gg_two_hop_rank).
// No embedding table is read: integer gathers over the SET adjacency of ensure_set_adjacency (pair_neighbors.hip).  The kernels
// hold no floating-point operation.
//
// Shape (the first build; what was not tuned is listed in DESIGN.md "Two-hop sweep").  The host plans per query from the host
// copy of the set adjacency: T(u) = sum over w in N(u) of deg(w), the entries of the expansion.  One workgroup per query:
//   fill        a (column, uint64 sum) SetTable (set_sweep.h) for min(T, n_node) entries.  T <= TH_LDS_CAP = 2048: the table lies
//               in LDS (4096 slots x 12 B = 48 KiB, with the selection's buffers 52 KiB: three workgroups share a CU's
//               160 KiB); above, in a zeroed table of the context's scratch buffer (per task the values, then the keys), the
//               queries batched under scratch_bytes.
//               Lists N(w) of up to TH_NARROW = 64 entries are walked by groups of 16 lanes (16 lists at a time), longer ones
//               by all 256 lanes of the workgroup: no list is truncated and no lane walks a hub's list alone;
//   rank        the target's slot is looked up, then the table is scanned once: eligibility is c != u, c != v plus, under
//               exclude = 2, a binary search in the sorted N(u); n_pos, ahead and pos_below are counted with compares, folded
//               per wavefront by shuffles and per workgroup through LDS;
//   top-K       the scan zeroes the values of the ineligible entries in place and folds n_pos and the largest score; if
//               n_pos > k a radix select on the composite key (score, ~column) -- 8 bits per pass from the first non-zero byte
//               of the largest score down, an LDS histogram with integer adds, the bucket found by a workgroup scan -- ends at
//               the first byte whose bucket holds exactly the entries still wanted; the min(k, n_pos) survivors are gathered
//               into LDS and bitonic-sorted (score descending, column ascending).  Composite keys are distinct, so selection and
//               order are exact.
// Every sum is an integer and the order is total, so a query's outputs depend on the graph, the weights and the query alone --
// not on the request, the grid, the batches, the order of the inserts or the run.
#include <algorithm>

#include "set_sweep.h"

namespace gg {

namespace {

constexpr int TH_LDS_CAP = 2048;      // expansion entries T the LDS table takes (Engine.TWO_HOP_LDS_CAP); larger queries use global memory
constexpr int TH_LDS_SLOTS = 2 * TH_LDS_CAP;
constexpr int TH_MAX_K = 256;         // list length at most: the survivors are sorted by one workgroup of 256 threads
constexpr int TH_NARROW = 64;         // a list N(w) up to this length is walked by a 16-lane group, a longer one by the workgroup
constexpr int TH_BLOCKS = 2048;       // workgroups per launch at most; they stride over the tasks behind them
constexpr int64_t TH_SCRATCH = 256ll << 20;  // default cap on the global tables of one pass, bytes
constexpr int64_t TH_CHUNK_OUT = 1ll << 23;  // list entries (queries x k) of one chunk of a top-K request at most

struct ThTask {
    int32_t q;        // query of the chunk
    uint32_t slots;   // table size, a power of two
    int64_t off;      // global table: first 8-byte word of the task's table in tab (slots values, then slots key words)
};

struct ThArgs {
    const ThTask *task;
    int n_task;
    unsigned long long *tab;          // zeroed global tables of the pass
    const int32_t *u, *v;             // [chunk] query nodes; targets (rank only)
    const int64_t *ptr;               // set adjacency
    const int32_t *adj;
    const unsigned long long *w;      // [n_node] or NULL: every weight 1
    int excl;                         // 1: c != u; 2: c outside N(u) + {u}
    int k;
    int32_t *out_col;                 // top-K: [chunk, k]
    unsigned long long *out_score;    //        [chunk, k]
    int32_t *n_pos;                   // [chunk]
    unsigned long long *score;        // rank: [chunk]
    int32_t *ahead, *pos_below;       //       [chunk]
};

template <bool GLOBAL>
using ThTab = SetTable<unsigned long long, GLOBAL>;  // at most min(T, n_node) distinct columns in >= twice as many slots

// x in the sorted list A[0, len)
__device__ __forceinline__ bool th_member(const int32_t *A, int len, int x) {
    const int p = set_lower_bound(A, 0, len, x);
    return p < len && A[p] == x;
}

// the expansion of u into the table; every thread of the workgroup calls it (barrier inside)
template <bool GLOBAL>
__device__ __forceinline__ void th_fill(const ThArgs &o, const ThTab<GLOBAL> &tb, int64_t ub, int du) {
    const int tid = threadIdx.x, gl = tid & 15;
    int wide = 0;
    for (int j = tid >> 4; j < du; j += 16) {
        const int w = o.adj[ub + j];
        const int64_t wb = o.ptr[w];
        const int dw = (int)(o.ptr[w + 1] - wb);
        if (dw > TH_NARROW) {
            wide = 1;
            continue;
        }
        const unsigned long long wv = o.w ? o.w[w] : 1ull;
        for (int e = gl; e < dw; e += 16) tb.add(o.adj[wb + e], wv);
    }
    if (__syncthreads_or(wide)) {  // (block-uniform)
        for (int j = 0; j < du; ++j) {
            const int w = o.adj[ub + j];
            const int64_t wb = o.ptr[w];
            const int dw = (int)(o.ptr[w + 1] - wb);
            if (dw <= TH_NARROW) continue;
            const unsigned long long wv = o.w ? o.w[w] : 1ull;
            for (int e = tid; e < dw; e += 256) tb.add(o.adj[wb + e], wv);
        }
    }
    tb.fill_done();
}

template <bool GLOBAL>
__global__ __launch_bounds__(256) void th_rank_kernel(ThArgs o) {
    __shared__ uint32_t s_key[GLOBAL ? 1 : TH_LDS_SLOTS];
    __shared__ unsigned long long s_val[GLOBAL ? 1 : TH_LDS_SLOTS];
    __shared__ int r_cnt[4][3];
    const int tid = threadIdx.x;
    for (int t = blockIdx.x; t < o.n_task; t += gridDim.x) {  // (block-uniform: the barriers below are reached by every thread)
        const ThTask tk = o.task[t];
        const int i = tk.q, u = o.u[i], v = o.v[i];
        ThTab<GLOBAL> tb;
        tb.val = GLOBAL ? o.tab + tk.off : s_val;
        tb.key = GLOBAL ? (uint32_t *)(tb.val + tk.slots) : s_key;
        tb.mask = tk.slots - 1u;
        if (!GLOBAL) tb.clear_lds();
        const int64_t ub = o.ptr[u];
        const int du = (int)(o.ptr[u + 1] - ub);
        th_fill<GLOBAL>(o, tb, ub, du);
        const unsigned long long sv = tb.find(v);  // (the same probes in every thread)
        int np = 0, ah = 0, below = 0;
        for (uint32_t s = tid; s < tk.slots; s += 256) {
            const uint32_t k = tb.ld_key(s);
            if (k == 0u) continue;
            const unsigned long long x = tb.ld_val(s);
            const int c = (int)(k - 1u);
            if (x == 0ull || c == u || c == v) continue;
            if (o.excl == 2 && th_member(o.adj + ub, du, c)) continue;
            ++np;
            ah += x > sv || (x == sv && c < v);
            below += c < v;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            np += __shfl_xor(np, off, 64);
            ah += __shfl_xor(ah, off, 64);
            below += __shfl_xor(below, off, 64);
        }
        if ((tid & 63) == 0) r_cnt[tid >> 6][0] = np, r_cnt[tid >> 6][1] = ah, r_cnt[tid >> 6][2] = below;
        __syncthreads();
        if (tid == 0) {
            o.score[i] = sv;
            o.n_pos[i] = r_cnt[0][0] + r_cnt[1][0] + r_cnt[2][0] + r_cnt[3][0];
            o.ahead[i] = r_cnt[0][1] + r_cnt[1][1] + r_cnt[2][1] + r_cnt[3][1];
            o.pos_below[i] = r_cnt[0][2] + r_cnt[1][2] + r_cnt[2][2] + r_cnt[3][2];
        }
        __syncthreads();  // (the next task clears the table and the fold words)
    }
}

// "a comes before b": score descending, column ascending
__device__ __forceinline__ bool th_before(unsigned long long sa, uint32_t ca, unsigned long long sb, uint32_t cb) {
    return sa > sb || (sa == sb && ca < cb);
}

template <bool GLOBAL>
__global__ __launch_bounds__(256) void th_topk_kernel(ThArgs o) {
    __shared__ uint32_t s_key[GLOBAL ? 1 : TH_LDS_SLOTS];
    __shared__ unsigned long long s_val[GLOBAL ? 1 : TH_LDS_SLOTS];
    __shared__ unsigned long long s_sc[TH_MAX_K], r_max[4], s_thr_hi;
    __shared__ uint32_t s_cl[TH_MAX_K], s_hist[256], r_sum[4], s_thr_lo, s_rem, s_n, s_done;
    const int tid = threadIdx.x;
    for (int t = blockIdx.x; t < o.n_task; t += gridDim.x) {  // (block-uniform: the barriers below are reached by every thread)
        const ThTask tk = o.task[t];
        const int i = tk.q, u = o.u[i];
        ThTab<GLOBAL> tb;
        tb.val = GLOBAL ? o.tab + tk.off : s_val;
        tb.key = GLOBAL ? (uint32_t *)(tb.val + tk.slots) : s_key;
        tb.mask = tk.slots - 1u;
        if (!GLOBAL) tb.clear_lds();
        const int64_t ub = o.ptr[u];
        const int du = (int)(o.ptr[u + 1] - ub);
        th_fill<GLOBAL>(o, tb, ub, du);
        // Every scan below gives slot s to thread s mod 256, so a thread reads back only the zeroes it stored itself.
        uint32_t np = 0;
        unsigned long long mx = 0ull;
        for (uint32_t s = tid; s < tk.slots; s += 256) {
            const uint32_t k = tb.ld_key(s);
            if (k == 0u) continue;
            const unsigned long long x = tb.ld_val(s);
            if (x == 0ull) continue;
            const int c = (int)(k - 1u);
            if (c == u || (o.excl == 2 && th_member(o.adj + ub, du, c))) {
                tb.clear_val(s);
                continue;
            }
            ++np;
            mx = max(mx, x);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            np += __shfl_xor(np, off, 64);
            mx = max(mx, (unsigned long long)__shfl_xor(mx, off, 64));
        }
        if ((tid & 63) == 0) r_sum[tid >> 6] = np, r_max[tid >> 6] = mx;
        s_sc[tid] = 0ull;  // (padding: score 0, column -1 -- behind every survivor)
        s_cl[tid] = 0xffffffffu;
        if (tid == 0) s_thr_hi = 0ull, s_thr_lo = 0u, s_rem = (uint32_t)o.k, s_n = 0u, s_done = 0u;
        __syncthreads();
        np = r_sum[0] + r_sum[1] + r_sum[2] + r_sum[3];
        mx = max(max(r_max[0], r_max[1]), max(r_max[2], r_max[3]));
        if (np > (uint32_t)o.k) {  // (block-uniform) the k-th largest composite key, byte by byte from the top
            for (int b = 4 + (63 - __clzll((long long)mx)) / 8; b >= 0; --b) {  // (mx > 0; bytes above b are zero in every score)
                s_hist[tid] = 0u;
                __syncthreads();  // (also: the threshold words of the pass before)
                const unsigned long long thi = s_thr_hi;
                const uint32_t tlo = s_thr_lo, rem = s_rem;
                for (uint32_t s = tid; s < tk.slots; s += 256) {
                    const uint32_t k = tb.ld_key(s);
                    if (k == 0u) continue;
                    const unsigned long long x = tb.ld_val(s);
                    if (x == 0ull) continue;
                    const uint32_t lo = ~(k - 1u);
                    bool match;
                    uint32_t byte;
                    if (b >= 4) {
                        const int sh = 8 * (b - 4);
                        match = sh == 56 || (x >> (sh + 8)) == (thi >> (sh + 8));
                        byte = (uint32_t)(x >> sh) & 255u;
                    } else {
                        const int sh = 8 * b;
                        match = x == thi && (b == 3 || (lo >> (sh + 8)) == (tlo >> (sh + 8)));
                        byte = (lo >> sh) & 255u;
                    }
                    if (match) atomicAdd(&s_hist[byte], 1u);
                }
                __syncthreads();
                // thread t takes bucket 255 - t: an inclusive scan over the threads counts the entries in its bucket and above
                const uint32_t h = s_hist[255 - tid];
                uint32_t incl = h;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t y = __shfl_up(incl, off, 64);
                    if ((tid & 63) >= off) incl += y;
                }
                if ((tid & 63) == 63) r_sum[tid >> 6] = incl;
                __syncthreads();
                for (int w = 0; w < (tid >> 6); ++w) incl += r_sum[w];
                if (incl >= rem && incl - h < rem) {  // (one thread: the bucket that holds the rem-th largest)
                    const uint32_t bucket = 255u - (uint32_t)tid, left = rem - (incl - h);
                    if (b >= 4) s_thr_hi = thi | ((unsigned long long)bucket << (8 * (b - 4)));
                    else s_thr_lo = tlo | (bucket << (8 * b));
                    s_rem = left;
                    s_done = h == left;  // the whole bucket survives: the bytes below stay zero
                }
                __syncthreads();
                if (s_done) break;  // (block-uniform; the last byte always ends here: the keys are distinct)
            }
        }
        const unsigned long long thi = s_thr_hi;
        const uint32_t tlo = s_thr_lo;
        for (uint32_t s = tid; s < tk.slots; s += 256) {
            const uint32_t k = tb.ld_key(s);
            if (k == 0u) continue;
            const unsigned long long x = tb.ld_val(s);
            if (x == 0ull) continue;
            const uint32_t lo = ~(k - 1u);
            if (x > thi || (x == thi && lo >= tlo)) {
                const uint32_t p = atomicAdd(&s_n, 1u);
                if (p < (uint32_t)TH_MAX_K) s_sc[p] = x, s_cl[p] = k - 1u;  // (p < min(k, n_pos) by the selection)
            }
        }
        __syncthreads();
        for (int k2 = 2; k2 <= TH_MAX_K; k2 <<= 1)
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                const int p = tid ^ j;
                if (p > tid) {
                    const bool up = (tid & k2) == 0;
                    const unsigned long long sa = s_sc[tid], sb = s_sc[p];
                    const uint32_t ca = s_cl[tid], cb = s_cl[p];
                    if (th_before(sb, cb, sa, ca) == up) s_sc[tid] = sb, s_cl[tid] = cb, s_sc[p] = sa, s_cl[p] = ca;
                }
                __syncthreads();
            }
        if (tid < o.k) {
            o.out_col[(int64_t)i * o.k + tid] = (int32_t)s_cl[tid];
            o.out_score[(int64_t)i * o.k + tid] = s_sc[tid];
        }
        if (tid == 0) o.n_pos[i] = (int32_t)np;
        __syncthreads();  // (the next task clears the table, the list and the fold words)
    }
}

// The sweep of one request: `rank` selects the outputs.  Queries go in chunks (bounded device memory for the outputs); within a
// chunk the LDS-table queries are one launch and the global-table queries as many passes as scratch_bytes asks for (a pass takes
// at least one query, whatever its table's size).
int th_run(gg_ctx *ctx, const char *fn, bool rank, const int32_t *u, const int32_t *v, int64_t m, int k, const uint64_t *weights, int excl, int64_t scratch_bytes,
           int32_t *out_col, uint64_t *out_score, uint64_t *score, int32_t *ahead, int32_t *n_pos, int32_t *pos_below, double *kernel_ms) {
    const int n = ctx->n_node;
    GG_HIP(ctx, hipSetDevice(ctx->device));
    int rc = ensure_set_adjacency(ctx);
    if (rc == GG_OK && weights) rc = check_weight_bound(ctx, fn, weights, n);
    if (rc != GG_OK) return rc;
    const int64_t cap = scratch_bytes > 0 ? scratch_bytes : TH_SCRATCH;
    const int64_t *hp = ctx->set.h_ptr.data();
    const int32_t *ha = ctx->set.h_adj.data();
    const int64_t chunk = rank ? std::min<int64_t>(m, 1 << 20) : std::min<int64_t>(m, std::max<int64_t>(1, TH_CHUNK_OUT / k));
    ScopedBuf d_u, d_v, d_w, d_task, d_col, d_sc, d_np, d_ah, d_below;
    hipError_t e = d_u.reserve(sizeof(int32_t) * (size_t)chunk);
    if (e == hipSuccess) e = d_np.reserve(sizeof(int32_t) * (size_t)chunk);
    if (e == hipSuccess) e = d_task.reserve(sizeof(ThTask) * (size_t)chunk);
    if (rank) {
        for (ScopedBuf *b : {&d_v, &d_ah, &d_below})
            if (e == hipSuccess) e = b->reserve(sizeof(int32_t) * (size_t)chunk);
        if (e == hipSuccess) e = d_sc.reserve(sizeof(uint64_t) * (size_t)chunk);
    } else {
        if (e == hipSuccess) e = d_col.reserve(sizeof(int32_t) * (size_t)chunk * k);
        if (e == hipSuccess) e = d_sc.reserve(sizeof(uint64_t) * (size_t)chunk * k);
    }
    if (e == hipSuccess && weights) e = d_w.reserve(sizeof(uint64_t) * (size_t)n);
    if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "%s: %s", fn, hipGetErrorString(e));
    if (weights) GG_HIP_FN(hipMemcpyAsync(d_w.p, weights, sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    std::vector<ThTask> task;
    std::vector<int64_t> expansion;   // T(u) of the chunk's queries
    std::vector<int64_t> pass_first;  // global-table passes: first task of each, then the end
    double ms_total = 0.0;
    for (int64_t p0 = 0; p0 < m; p0 += chunk) {
        const int cr = (int)std::min<int64_t>(chunk, m - p0);
        // the chunk's tasks: the LDS-table queries first, then the global-table queries cut into passes
        task.assign((size_t)cr, ThTask{});
        expansion.resize((size_t)cr);
        for (int i = 0; i < cr; ++i) {
            const int a = u[p0 + i];
            int64_t T = 0;
            for (int64_t j = hp[a]; j < hp[a + 1]; ++j) T += hp[ha[j] + 1] - hp[ha[j]];
            expansion[(size_t)i] = T;
        }
        int n_lds = 0, n_glob = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (int i = 0; i < cr; ++i) {
                const int64_t T = expansion[(size_t)i];
                const bool lds = T <= TH_LDS_CAP;
                if (lds != (pass == 0)) continue;
                ThTask &tk = task[(size_t)(lds ? n_lds++ : n_lds + n_glob++)];
                tk.q = i;
                tk.slots = (uint32_t)set_table_slots(std::min<int64_t>(T, n));
            }
        pass_first.assign(1, n_lds);
        int64_t words = 0, max_words = 0;
        for (int t = n_lds; t < cr; ++t) {
            const int64_t need = (int64_t)task[t].slots + task[t].slots / 2;  // 8-byte words: the values, then the 4-byte keys
            if (words && (words + need) * 8 > cap) {
                pass_first.push_back(t);
                words = 0;
            }
            task[t].off = words;
            words += need;
            max_words = std::max(max_words, words);
        }
        pass_first.push_back(cr);
        if (max_words) {
            e = ctx->set.th_tab.reserve(sizeof(uint64_t) * (size_t)max_words);
            if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "%s: %lld bytes of table scratch: %s", fn, (long long)(max_words * 8), hipGetErrorString(e));
        }
        GG_HIP_FN(hipMemcpyAsync(d_u.p, u + p0, sizeof(int32_t) * cr, hipMemcpyHostToDevice, ctx->stream));
        if (rank) GG_HIP_FN(hipMemcpyAsync(d_v.p, v + p0, sizeof(int32_t) * cr, hipMemcpyHostToDevice, ctx->stream));
        GG_HIP_FN(hipMemcpyAsync(d_task.p, task.data(), sizeof(ThTask) * (size_t)cr, hipMemcpyHostToDevice, ctx->stream));
        ThArgs o{};
        o.tab = ctx->set.th_tab.as<unsigned long long>();
        o.u = d_u.as<int32_t>();
        o.v = d_v.as<int32_t>();
        o.ptr = ctx->set.ptr.as<int64_t>();
        o.adj = ctx->set.adj.as<int32_t>();
        o.w = weights ? d_w.as<unsigned long long>() : nullptr;
        o.excl = excl;
        o.k = k;
        o.out_col = d_col.as<int32_t>();
        o.out_score = rank ? nullptr : d_sc.as<unsigned long long>();
        o.score = rank ? d_sc.as<unsigned long long>() : nullptr;
        o.n_pos = d_np.as<int32_t>();
        o.ahead = d_ah.as<int32_t>();
        o.pos_below = d_below.as<int32_t>();
        (void)hipEventRecord(ctx->ev0, ctx->stream);
        if (n_lds) {
            o.task = d_task.as<ThTask>();
            o.n_task = n_lds;
            const dim3 grid((unsigned)std::min(TH_BLOCKS, n_lds));
            if (rank) hipLaunchKernelGGL(th_rank_kernel<false>, grid, dim3(256), 0, ctx->stream, o);
            else hipLaunchKernelGGL(th_topk_kernel<false>, grid, dim3(256), 0, ctx->stream, o);
        }
        for (size_t ps = 0; ps + 1 < pass_first.size(); ++ps) {
            const int64_t t0 = pass_first[ps], t1 = pass_first[ps + 1];
            if (t1 == t0) continue;
            const int64_t used = task[(size_t)t1 - 1].off + task[(size_t)t1 - 1].slots + task[(size_t)t1 - 1].slots / 2;
            GG_HIP_FN(hipMemsetAsync(ctx->set.th_tab.p, 0, sizeof(uint64_t) * (size_t)used, ctx->stream));
            o.task = d_task.as<ThTask>() + t0;
            o.n_task = (int)(t1 - t0);
            const dim3 grid((unsigned)std::min<int64_t>(TH_BLOCKS, t1 - t0));
            if (rank) hipLaunchKernelGGL(th_rank_kernel<true>, grid, dim3(256), 0, ctx->stream, o);
            else hipLaunchKernelGGL(th_topk_kernel<true>, grid, dim3(256), 0, ctx->stream, o);
        }
        (void)hipEventRecord(ctx->ev1, ctx->stream);
        GG_HIP_FN(hipGetLastError());
        GG_HIP_FN(hipMemcpyAsync(n_pos + p0, d_np.p, sizeof(int32_t) * cr, hipMemcpyDeviceToHost, ctx->stream));
        if (rank) {
            GG_HIP_FN(hipMemcpyAsync(score + p0, d_sc.p, sizeof(uint64_t) * cr, hipMemcpyDeviceToHost, ctx->stream));
            GG_HIP_FN(hipMemcpyAsync(ahead + p0, d_ah.p, sizeof(int32_t) * cr, hipMemcpyDeviceToHost, ctx->stream));
            GG_HIP_FN(hipMemcpyAsync(pos_below + p0, d_below.p, sizeof(int32_t) * cr, hipMemcpyDeviceToHost, ctx->stream));
        } else {
            GG_HIP_FN(hipMemcpyAsync(out_col + p0 * k, d_col.p, sizeof(int32_t) * (size_t)cr * k, hipMemcpyDeviceToHost, ctx->stream));
            GG_HIP_FN(hipMemcpyAsync(out_score + p0 * k, d_sc.p, sizeof(uint64_t) * (size_t)cr * k, hipMemcpyDeviceToHost, ctx->stream));
        }
        GG_HIP_FN(hipStreamSynchronize(ctx->stream));
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
        ms_total += ms;
    }
    if (kernel_ms) *kernel_ms = ms_total;
    return GG_OK;
}

// the argument checks the two entry points share, in the order the header lists their texts
int th_check(gg_ctx *ctx, const char *fn, int64_t m, const char *m_name, int exclude, int64_t scratch_bytes) {
    GG_CHECK(ctx, ctx->g_rowptr, GG_EINVAL, "%s: needs the training graph (gg_set_graph_csr)", fn);
    GG_CHECK(ctx, m >= 0, GG_EINVAL, "%s: %s = %lld is negative", fn, m_name, (long long)m);
    GG_CHECK(ctx, m <= 0x7fffffffLL, GG_EINVAL, "%s: %s = %lld does not fit in 31 bits", fn, m_name, (long long)m);
    GG_CHECK(ctx, exclude == 1 || exclude == 2, GG_EINVAL, "%s: exclude = %d is neither 1 (self) nor 2 (graph)", fn, exclude);
    GG_CHECK(ctx, scratch_bytes >= 0, GG_EINVAL, "%s: scratch_bytes = %lld is negative", fn, (long long)scratch_bytes);
    return GG_OK;
}

}  // namespace

}  // namespace gg

using namespace gg;

// gg_two_hop_topk, gg_two_hop_rank: see include/graphgan_hip.h.
extern "C" int gg_two_hop_topk(gg_ctx *ctx, const int32_t *rows, int64_t n_rows, int32_t k, const uint64_t *weights, int32_t exclude, int64_t scratch_bytes,
                               int32_t *out_col, uint64_t *out_score, int32_t *n_pos, double *kernel_ms) {
    const char *fn = "gg_two_hop_topk";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (kernel_ms) *kernel_ms = 0.0;
    const int rc = th_check(ctx, fn, n_rows, "n_rows", exclude, scratch_bytes);
    if (rc != GG_OK) return rc;
    GG_CHECK(ctx, k >= 1 && k <= TH_MAX_K, GG_EINVAL, "%s: k = %d outside [1, %d]", fn, k, TH_MAX_K);
    if (n_rows == 0) return GG_OK;
    GG_CHECK(ctx, rows && out_col && out_score && n_pos, GG_EINVAL, "%s: rows, out_col, out_score and n_pos must not be NULL", fn);
    const int rc2 = check_ids(ctx, fn, "rows", rows, n_rows);
    if (rc2 != GG_OK) return rc2;
    return th_run(ctx, fn, false, rows, nullptr, n_rows, k, weights, exclude, scratch_bytes, out_col, out_score, nullptr, nullptr, n_pos, nullptr, kernel_ms);
}

extern "C" int gg_two_hop_rank(gg_ctx *ctx, const int32_t *u, const int32_t *v, int64_t m, const uint64_t *weights, int32_t exclude, int64_t scratch_bytes,
                               uint64_t *score, int32_t *ahead, int32_t *n_pos, int32_t *pos_below, double *kernel_ms) {
    const char *fn = "gg_two_hop_rank";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (kernel_ms) *kernel_ms = 0.0;
    const int rc = th_check(ctx, fn, m, "m", exclude, scratch_bytes);
    if (rc != GG_OK) return rc;
    if (m == 0) return GG_OK;
    GG_CHECK(ctx, u && v && score && ahead && n_pos && pos_below, GG_EINVAL, "%s: u, v, score, ahead, n_pos and pos_below must not be NULL", fn);
    int rc2 = check_ids(ctx, fn, "u", u, m);
    if (rc2 == GG_OK) rc2 = check_ids(ctx, fn, "v", v, m);
    if (rc2 != GG_OK) return rc2;
    return th_run(ctx, fn, true, u, v, m, 1, weights, exclude, scratch_bytes, nullptr, nullptr, score, ahead, n_pos, pos_below, kernel_ms);
}
