// two_hop_pairs.hip -- the two-hop pair sweep: the k best unordered pairs {u, v}, u < v, of a node set under
// S(u, v) = sum over w in N(u) & N(v) of weights[w] on the SET adjacency of the resident training graph (unsigned 64-bit integers;
// no weights: common neighbours), optionally without the pairs that are edges.  The graph-only line beside gg_top_pairs: the same
// consumer shape -- one global floor, a device append buffer, a selection on the host -- on the filled table of the two-hop sweep
// (two_hop.hip) in place of the tile stream.  No embedding table is read; the kernels hold no floating-point operation.
//
// Order: (S, u, v) is ahead of (S', u', v') when S > S' || (S == S' && (u < u' || (u == u' && v < v'))): total and integer.
//
// Device side.  One workgroup of 256 threads per source u, striding over the tasks of a launch:
//   fill        the expansion of u restricted to the upper triangle: for w in N(u) only the suffix of the sorted N(w) with c > u
//               (one set_lower_bound per list) is added to a (column, uint64 sum) SetTable.  The host plans from
//               T'(u) = sum over w in N(u) of |{c in N(w), c > u}|: T' <= THP_LDS_CAP: the table lies in LDS, above in a zeroed
//               table of the context's scratch buffer, the sources batched under scratch_bytes.  Lists of up to THP_NARROW entries
//               are walked by groups of 16 lanes, longer ones by the whole workgroup;
//   consume     set_floor_consume (set_consume.h): one scan against the floor, survivors appended to the global buffer.
//
// Host schedule (PairSweep; the shape of top_pairs.hip's PairRun).  The sources -- the members with T' > 0 -- go in descending
// B(u) = sum over w in N(u) of weights[w] (deg(u) without weights), ties by id: S(u, .) <= B(u), so the floor rises early, and a
// source with B(u) < fs is not launched at all (exact: nothing of it can be ahead of the floor).  A launch is a batch of
// consecutive sources: its LDS-table kernel and its global-table passes, then ONE 4-byte read-back of the fill counter.  Overflow:
// the counter goes back to its value before the launch, the buffer is compacted if it holds more than k entries, and the batch is
// rerun as two halves (a single source: once more behind the compaction; it always fits behind k entries, hence buffer_entries
// >= k + the largest min(T'(u), members above u)).  Batches start at 256 sources and double while nothing overflows.  A compaction
// (fill above compact_above(), and at the end) selects the k best entries on the host and stores the k-th as the new floor.  The
// floor only ever drops pairs that k known pairs are ahead of, so the result is exact and a function of the graph, the weights,
// the set, k and exclude alone -- not of the buffer, the scratch cap, the batches, the source order or the order of the appends.
#include <algorithm>
#include <vector>

#include "set_consume.h"

namespace gg {

namespace {

// the shape of the two-hop sweep (two_hop.hip: TH_LDS_CAP, TH_NARROW, TH_BLOCKS, TH_SCRATCH), kept in step by tests/test_graph_pairs_cpu.py
constexpr int THP_LDS_CAP = 2048;      // expansion entries T' the LDS table takes (Engine.TWO_HOP_LDS_CAP); larger sources use global memory
constexpr int THP_LDS_SLOTS = 2 * THP_LDS_CAP;
constexpr int THP_NARROW = 64;         // a list N(w) up to this length is walked by a 16-lane group, a longer one by the workgroup
constexpr int THP_BLOCKS = 2048;       // workgroups per launch at most; they stride over the tasks behind them
constexpr int64_t THP_SCRATCH = 256ll << 20;  // default cap on the global tables of one pass, bytes
constexpr int64_t THP_MAX_K = 1 << 20;
constexpr int64_t THP_MIN_BUF = 1 << 22, THP_MAX_BUF = 1 << 26;  // the default's floor and the ceiling: those of gg_top_pairs
constexpr int64_t THP_FIRST_BATCH = 256, THP_MAX_BATCH = 1 << 16;  // sources of the first and of the largest batch
constexpr int64_t THP_MAX_ENTRIES = int64_t(1) << 30;  // entries of one table at most: twice as many slots fit the 32-bit slot count
constexpr int64_t THP_BUF_LIMIT = int64_t(1) << 31;  // no buffer is larger: a batch is cut where its appends could wrap the 32-bit fill counter

struct ThpTask {
    int32_t u;        // the source
    uint32_t slots;   // table size, a power of two
    int64_t off;      // global table: first 8-byte word of the task's table in tab (slots values, then slots key words)
};

struct ThpArgs {
    const ThpTask *task;
    int n_task;
    unsigned long long *tab;          // zeroed global tables of the pass
    const int64_t *ptr;               // set adjacency
    const int32_t *adj;
    const unsigned long long *w;      // [n_node] or NULL: every weight 1
    int excl;                         // 1: v outside N(u)
    const uint32_t *floor;            // [4] fs lo, fs hi, fu, fv
    SetFloor out;                     // (its floor is read from `floor` by the kernel)
};

template <bool GLOBAL>
using ThpTab = SetTable<unsigned long long, GLOBAL>;  // at most min(T', n_node - 1 - u) distinct columns in >= twice as many slots

// the expansion of u above u into the table; every thread of the workgroup calls it (barrier inside)
template <bool GLOBAL>
__device__ __forceinline__ void thp_fill(const ThpArgs &o, const ThpTab<GLOBAL> &tb, int u, int64_t ub, int du) {
    const int tid = threadIdx.x, gl = tid & 15;
    int wide = 0;
    for (int j = tid >> 4; j < du; j += 16) {
        const int w = o.adj[ub + j];
        const int64_t wb = o.ptr[w];
        const int dw = (int)(o.ptr[w + 1] - wb);
        if (dw > THP_NARROW) {
            wide = 1;
            continue;
        }
        const unsigned long long wv = o.w ? o.w[w] : 1ull;
        for (int e = set_lower_bound(o.adj + wb, 0, dw, u + 1) + gl; e < dw; e += 16) tb.add(o.adj[wb + e], wv);
    }
    if (__syncthreads_or(wide)) {  // (block-uniform)
        for (int j = 0; j < du; ++j) {
            const int w = o.adj[ub + j];
            const int64_t wb = o.ptr[w];
            const int dw = (int)(o.ptr[w + 1] - wb);
            if (dw <= THP_NARROW) continue;
            const unsigned long long wv = o.w ? o.w[w] : 1ull;
            for (int e = set_lower_bound(o.adj + wb, 0, dw, u + 1) + tid; e < dw; e += 256) tb.add(o.adj[wb + e], wv);
        }
    }
    tb.fill_done();
}

template <bool GLOBAL, bool BM>
__global__ __launch_bounds__(256) void thp_kernel(ThpArgs o) {
    __shared__ uint32_t s_key[GLOBAL ? 1 : THP_LDS_SLOTS];
    __shared__ unsigned long long s_val[GLOBAL ? 1 : THP_LDS_SLOTS];
    SetFloor f = o.out;
    f.fs = ((unsigned long long)o.floor[1] << 32) | o.floor[0];
    f.fu = (int)o.floor[2];
    f.fv = (int)o.floor[3];
    for (int t = blockIdx.x; t < o.n_task; t += gridDim.x) {  // (block-uniform: the barriers below are reached by every thread)
        const ThpTask tk = o.task[t];
        const int u = tk.u;
        ThpTab<GLOBAL> tb;
        tb.val = GLOBAL ? o.tab + tk.off : s_val;
        tb.key = GLOBAL ? (uint32_t *)(tb.val + tk.slots) : s_key;
        tb.mask = tk.slots - 1u;
        if (!GLOBAL) tb.clear_lds();
        const int64_t ub = o.ptr[u];
        const int du = (int)(o.ptr[u + 1] - ub);
        thp_fill<GLOBAL>(o, tb, u, ub, du);
        set_floor_consume<GLOBAL, BM>(tb, tk.slots, u, o.adj + ub, du, o.excl, f);
        __syncthreads();  // (the next task clears the table)
    }
}

struct Entry {
    uint32_t lo, hi, u, v;
    uint64_t s() const { return ((uint64_t)hi << 32) | lo; }
};
inline bool entry_ahead(const Entry &a, const Entry &b) {
    if (a.s() != b.s()) return a.s() > b.s();
    if (a.u != b.u) return a.u < b.u;
    return a.v < b.v;
}

struct Source {
    int32_t u;
    uint64_t B;       // the skip bound
    int64_t T;        // T'(u)
    int64_t bound;    // min(T', members above u): the entries the source can append at most
};

// The whole run behind the checks.
struct PairSweep {
    gg_ctx *ctx;
    ThpArgs o;
    bool bitmap;
    int64_t k, cap, scratch;
    int n_node;
    const std::vector<Source> *src;
    ThpTask *d_task;
    uint32_t *d_floor;
    uint64_t fs = 0;         // the floor's score, as the host knows it (0: fewer than k pairs known)
    int64_t fill = 0;        // the device counter, as the host knows it
    int64_t launches = 0, retries = 0, compactions = 0, appended = 0, swept = 0, skipped = 0;
    std::vector<Entry> h;
    std::vector<ThpTask> task;
    hipError_t e = hipSuccess;
    bool internal = false;   // a single source did not fit behind k entries: cannot happen
    int64_t tab_fail = 0;    // bytes of table scratch that could not be reserved

    // fill above this: compact (top_pairs.hip's rule)
    int64_t compact_above() const { return std::min(k + (cap - k) / 2, std::max<int64_t>(3 * k, int64_t(1) << 16)); }

    // the fill entries of the buffer to the host, the k best kept and written back, the k-th as the new floor; sorted only at the end
    void compact(bool last = false) {
        h.resize((size_t)fill);
        if (fill) e = hipMemcpyAsync(h.data(), o.out.buf, sizeof(Entry) * (size_t)fill, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return;
        const size_t keep = (size_t)std::min<int64_t>(fill, k);
        if (keep) std::nth_element(h.begin(), h.begin() + (keep - 1), h.end(), entry_ahead);  // the keep-th best at keep - 1, the better ones in front
        h.resize(keep);
        ++compactions;
        if (last) {
            std::sort(h.begin(), h.end(), entry_ahead);
            return;
        }
        uint32_t head[5] = {0u, 0u, 0x7fffffffu, 0x7fffffffu, (uint32_t)keep};  // the floor (nothing is behind it), then the counter
        if ((int64_t)keep == k) {
            head[0] = h[keep - 1].lo, head[1] = h[keep - 1].hi, head[2] = h[keep - 1].u, head[3] = h[keep - 1].v;
            fs = h[keep - 1].s();
        }
        if (keep) e = hipMemcpyAsync(o.out.buf, h.data(), sizeof(Entry) * keep, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_floor, head, sizeof(head), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        fill = (int64_t)keep;
    }

    // The kernels of the sources [a, b) that the bound does not skip: the LDS-table sources in one launch, the global-table sources in
    // as many passes as `scratch` asks for (a pass takes at least one source, whatever its table's size).  -> the sources launched
    int64_t enqueue(int64_t a, int64_t b, int64_t &n_skip) {
        const std::vector<Source> &S = *src;
        task.clear();
        n_skip = 0;
        int n_lds = 0;
        for (int pass = 0; pass < 2; ++pass) {
            for (int64_t i = a; i < b; ++i) {
                if (S[(size_t)i].B < fs) {
                    n_skip += pass == 0;
                    continue;
                }
                if ((S[(size_t)i].T <= THP_LDS_CAP) != (pass == 0)) continue;
                ThpTask tk{};
                tk.u = S[(size_t)i].u;
                tk.slots = (uint32_t)set_table_slots(std::min<int64_t>(S[(size_t)i].T, (int64_t)n_node - 1 - tk.u));
                task.push_back(tk);
            }
            if (pass == 0) n_lds = (int)task.size();
        }
        const int n_all = (int)task.size();
        if (n_all == 0) return 0;
        std::vector<int> pass_first(1, n_lds);
        int64_t words = 0, max_words = 0;
        for (int t = n_lds; t < n_all; ++t) {
            const int64_t need = (int64_t)task[(size_t)t].slots + task[(size_t)t].slots / 2;  // 8-byte words: the values, then the 4-byte keys
            if (words && (words + need) * 8 > scratch) {
                pass_first.push_back(t);
                words = 0;
            }
            task[(size_t)t].off = words;
            words += need;
            max_words = std::max(max_words, words);
        }
        pass_first.push_back(n_all);
        if (max_words) {
            e = ctx->set.th_tab.reserve(sizeof(uint64_t) * (size_t)max_words);
            if (e != hipSuccess) {
                tab_fail = max_words * 8;
                return 0;
            }
        }
        e = hipMemcpyAsync(d_task, task.data(), sizeof(ThpTask) * (size_t)n_all, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return 0;
        ThpArgs args = o;
        args.tab = ctx->set.th_tab.as<unsigned long long>();
        if (n_lds) {
            args.task = d_task;
            args.n_task = n_lds;
            const dim3 grid((unsigned)std::min(THP_BLOCKS, n_lds));
            if (bitmap) hipLaunchKernelGGL((thp_kernel<false, true>), grid, dim3(256), 0, ctx->stream, args);
            else hipLaunchKernelGGL((thp_kernel<false, false>), grid, dim3(256), 0, ctx->stream, args);
        }
        for (size_t ps = 0; ps + 1 < pass_first.size(); ++ps) {
            const int t0 = pass_first[ps], t1 = pass_first[ps + 1];
            if (t1 == t0) continue;
            const int64_t used = task[(size_t)t1 - 1].off + task[(size_t)t1 - 1].slots + task[(size_t)t1 - 1].slots / 2;
            e = hipMemsetAsync(ctx->set.th_tab.p, 0, sizeof(uint64_t) * (size_t)used, ctx->stream);
            if (e != hipSuccess) return 0;
            args.task = d_task + t0;
            args.n_task = t1 - t0;
            const dim3 grid((unsigned)std::min(THP_BLOCKS, t1 - t0));
            if (bitmap) hipLaunchKernelGGL((thp_kernel<true, true>), grid, dim3(256), 0, ctx->stream, args);
            else hipLaunchKernelGGL((thp_kernel<true, false>), grid, dim3(256), 0, ctx->stream, args);
        }
        return n_all;
    }

    void run(int64_t a, int64_t b) {
        for (bool again = true; again;) {
            again = false;
            if (e != hipSuccess || internal || tab_fail || a >= b) return;
            int64_t n_skip = 0;
            const int64_t n_run = enqueue(a, b, n_skip);
            if (e != hipSuccess || tab_fail) return;
            if (n_run == 0) {
                skipped += n_skip;
                return;
            }
            ++launches;
            e = hipGetLastError();
            uint32_t now = 0;
            if (e == hipSuccess) e = hipMemcpyAsync(&now, o.out.fill, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) return;
            if ((int64_t)now <= cap) {
                appended += (int64_t)now - fill;
                fill = now;
                swept += n_run;
                skipped += n_skip;
                if (fill > compact_above()) compact();
                return;
            }
            // overflow: the counter back to its value before the launch, then the halves
            ++retries;
            const uint32_t before = (uint32_t)fill;
            e = hipMemcpyAsync(o.out.fill, &before, sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) return;
            const bool compacted = fill > k;
            if (compacted) compact();
            if (b - a > 1) {
                const int64_t mid = a + (b - a) / 2;
                run(a, mid);
                run(mid, b);
            } else if (compacted) {
                again = true;  // the one source once more, now behind at most k entries
            } else {
                internal = true;
            }
        }
    }

    // every batch of the source order: the first holds THP_FIRST_BATCH sources, the batch doubles while nothing overflows
    void sweep() {
        const std::vector<Source> &S = *src;
        const int64_t n_src = (int64_t)S.size();
        const int64_t max_append = (int64_t(1) << 32) - 1 - cap;  // (>= 2^31 - 1: above every single source's bound)
        int64_t batch = THP_FIRST_BATCH;
        for (int64_t a = 0; a < n_src && e == hipSuccess && !internal && !tab_fail;) {
            if (S[(size_t)a].B < fs) {  // (descending B: every source from here on is skipped)
                skipped += n_src - a;
                break;
            }
            int64_t b = a, sum = 0;
            while (b < n_src && b - a < batch && (b == a || sum + S[(size_t)b].bound <= max_append)) sum += S[(size_t)b++].bound;
            const int64_t r0 = retries;
            run(a, b);
            if (retries == r0) batch = std::min(batch * 2, THP_MAX_BATCH);
            a = b;
        }
    }
};

}  // namespace

}  // namespace gg

using namespace gg;

// gg_two_hop_top_pairs: see include/graphgan_hip.h.
extern "C" int gg_two_hop_top_pairs(gg_ctx *ctx, const int32_t *nodes, int64_t m, int64_t k, const uint64_t *weights, int32_t exclude, int64_t scratch_bytes,
                                    int64_t buffer_entries, int32_t *out_u, int32_t *out_v, uint64_t *out_score, int64_t *n_found, int64_t *stats,
                                    double *kernel_ms) {
    const char *fn = "gg_two_hop_top_pairs";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (kernel_ms) *kernel_ms = 0.0;
    GG_CHECK(ctx, ctx->g_rowptr, GG_EINVAL, "%s: needs the training graph (gg_set_graph_csr)", fn);
    GG_CHECK(ctx, k >= 1 && k <= THP_MAX_K, GG_EINVAL, "%s: k = %lld outside [1, 2^20]", fn, (long long)k);
    GG_CHECK(ctx, exclude == 0 || exclude == 1, GG_EINVAL, "%s: exclude = %d is neither 0 nor 1", fn, exclude);
    GG_CHECK(ctx, scratch_bytes >= 0, GG_EINVAL, "%s: scratch_bytes = %lld is negative", fn, (long long)scratch_bytes);
    GG_CHECK(ctx, buffer_entries >= 0, GG_EINVAL, "%s: buffer_entries = %lld is negative", fn, (long long)buffer_entries);
    GG_CHECK(ctx, out_u && out_v && out_score && n_found, GG_EINVAL, "%s: out_u, out_v, out_score and n_found must not be NULL", fn);
    const int n = ctx->n_node;
    if (nodes) {
        GG_CHECK(ctx, m >= 0, GG_EINVAL, "%s: m = %lld is negative", fn, (long long)m);
        for (int64_t i = 0; i < m; ++i) {
            GG_CHECK(ctx, nodes[i] >= 0 && nodes[i] < n, GG_EINVAL, "%s: nodes[%lld] = %d out of range [0, %d)", fn, (long long)i, nodes[i], n);
            GG_CHECK(ctx, i == 0 || nodes[i] > nodes[i - 1], GG_EINVAL, "%s: nodes[%lld] = %d is not above nodes[%lld] = %d (strictly ascending ids)", fn,
                     (long long)i, nodes[i], (long long)(i - 1), nodes[i - 1]);
        }
    } else {
        m = n;
    }
    GG_HIP(ctx, hipSetDevice(ctx->device));
    int rc = ensure_set_adjacency(ctx);
    if (rc == GG_OK && weights) rc = check_weight_bound(ctx, fn, weights, n);
    if (rc != GG_OK) return rc;
    // the plan, from the host copy of the set adjacency: T'(u) for every node in one pass over the lists (entry i of a sorted list
    // of d entries has d - 1 - i entries above it), B(u), and per member the entries it can append at most
    const int64_t *hp = ctx->set.h_ptr.data();
    const int32_t *ha = ctx->set.h_adj.data();
    std::vector<int64_t> T((size_t)n, 0);
    for (int w = 0; w < n; ++w) {
        const int64_t b = hp[w], d = hp[w + 1] - b;
        for (int64_t i = 0; i < d; ++i) T[(size_t)ha[b + i]] += d - 1 - i;
    }
    std::vector<Source> src;
    src.reserve((size_t)m);
    int64_t max_bound = 0, max_entries = 0;  // (max_entries: the distinct columns a table may have to take)
    for (int64_t i = 0; i < m; ++i) {
        const int32_t u = nodes ? nodes[i] : (int32_t)i;
        if (T[(size_t)u] == 0) continue;
        Source s;
        s.u = u;
        s.T = T[(size_t)u];
        s.bound = std::min<int64_t>(s.T, m - 1 - i);
        s.B = 0;
        if (weights) for (int64_t j = hp[u]; j < hp[u + 1]; ++j) s.B += weights[ha[j]];
        else s.B = (uint64_t)(hp[u + 1] - hp[u]);
        if (s.bound == 0) continue;
        max_bound = std::max(max_bound, s.bound);
        max_entries = std::max(max_entries, std::min<int64_t>(s.T, (int64_t)n - 1 - u));
        src.push_back(s);
    }
    GG_CHECK(ctx, max_entries <= THP_MAX_ENTRIES, GG_ECAPACITY, "%s: one source reaches %lld nodes above it, more than 2^30: its table has no 32-bit slot count", fn,
             (long long)max_entries);
    const int64_t min_buf = k + max_bound;
    GG_CHECK(ctx, min_buf <= THP_BUF_LIMIT, GG_ECAPACITY, "%s: one source can append %lld entries: a buffer of more than 2^31 entries", fn, (long long)max_bound);
    GG_CHECK(ctx, buffer_entries == 0 || (buffer_entries >= min_buf && buffer_entries <= std::max(THP_MAX_BUF, min_buf)), GG_EINVAL,
             "%s: buffer_entries = %lld outside [%lld, %lld] (0: the default; the minimum is k + %lld, the most entries one source can append)", fn,
             (long long)buffer_entries, (long long)min_buf, (long long)std::max(THP_MAX_BUF, min_buf), (long long)max_bound);
    for (int64_t i = 0; i < k; ++i) { out_u[i] = -1; out_v[i] = -1; out_score[i] = 0; }
    *n_found = 0;
    if (stats) for (int i = 0; i < 6; ++i) stats[i] = 0;
    if (src.empty()) return GG_OK;
    std::sort(src.begin(), src.end(), [](const Source &a, const Source &b) { return a.B != b.B ? a.B > b.B : a.u < b.u; });
    const int64_t cap = buffer_entries ? buffer_entries : std::max(min_buf, std::max<int64_t>(THP_MIN_BUF, 4 * k));
    const int n_words = cdiv(n, 32);
    ScopedBuf d_member, d_head, d_buf, d_w, d_task;
    std::vector<uint32_t> member;
    hipError_t e = d_head.reserve(sizeof(uint32_t) * 5);
    if (e == hipSuccess) e = d_buf.reserve(sizeof(Entry) * (size_t)cap);
    if (e == hipSuccess) e = d_task.reserve(sizeof(ThpTask) * (size_t)std::min<int64_t>((int64_t)src.size(), THP_MAX_BATCH));
    if (e == hipSuccess && nodes) e = d_member.reserve(sizeof(uint32_t) * (size_t)n_words);
    if (e == hipSuccess && weights) e = d_w.reserve(sizeof(uint64_t) * (size_t)n);
    if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "%s: %s", fn, hipGetErrorString(e));
    if (nodes) {
        member.assign((size_t)n_words, 0u);
        for (int64_t i = 0; i < m; ++i) member[(size_t)(nodes[i] >> 5)] |= 1u << (nodes[i] & 31);
        e = hipMemcpyAsync(d_member.p, member.data(), sizeof(uint32_t) * (size_t)n_words, hipMemcpyHostToDevice, ctx->stream);
    }
    if (e == hipSuccess && weights) e = hipMemcpyAsync(d_w.p, weights, sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream);
    const uint32_t head[5] = {0u, 0u, 0x7fffffffu, 0x7fffffffu, 0u};  // the floor: nothing is behind it; the counter at 0
    if (e == hipSuccess) e = hipMemcpyAsync(d_head.p, head, sizeof(head), hipMemcpyHostToDevice, ctx->stream);
    PairSweep R;
    R.ctx = ctx;
    R.bitmap = nodes != nullptr;
    R.k = k;
    R.cap = cap;
    R.scratch = scratch_bytes > 0 ? scratch_bytes : THP_SCRATCH;
    R.n_node = n;
    R.src = &src;
    R.d_task = d_task.as<ThpTask>();
    R.d_floor = d_head.as<uint32_t>();
    R.o = ThpArgs{};
    R.o.ptr = ctx->set.ptr.as<int64_t>();
    R.o.adj = ctx->set.adj.as<int32_t>();
    R.o.w = weights ? d_w.as<unsigned long long>() : nullptr;
    R.o.excl = exclude;
    R.o.floor = d_head.as<uint32_t>();
    R.o.out = SetFloor{0ull, 0, 0, d_member.as<uint32_t>(), d_head.as<uint32_t>() + 4, (uint32_t)cap, d_buf.as<uint4>()};
    R.e = e;
    if (e == hipSuccess) (void)hipEventRecord(ctx->ev0, ctx->stream);
    if (e == hipSuccess) R.sweep();
    if (R.e == hipSuccess && !R.internal && !R.tab_fail) R.compact(true);  // the k best, sorted, in R.h
    if (R.e == hipSuccess) (void)hipEventRecord(ctx->ev1, ctx->stream);
    if (R.e == hipSuccess) R.e = hipStreamSynchronize(ctx->stream);
    else (void)hipStreamSynchronize(ctx->stream);  // (the weights' source and the buffers go away behind it)
    if (R.tab_fail) return fail(ctx, GG_ENOMEM, "%s: %lld bytes of table scratch: %s", fn, (long long)R.tab_fail, hipGetErrorString(R.e));
    if (R.e != hipSuccess) return fail(ctx, GG_EHIP, "%s: %s", fn, hipGetErrorString(R.e));
    if (R.internal) return fail(ctx, GG_ECAPACITY, "%s: internal error: one source overflowed a buffer of %lld entries behind %lld", fn, (long long)cap, (long long)k);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    for (size_t i = 0; i < R.h.size(); ++i) {
        out_u[i] = (int32_t)R.h[i].u;
        out_v[i] = (int32_t)R.h[i].v;
        out_score[i] = R.h[i].s();
    }
    *n_found = (int64_t)R.h.size();
    if (stats) {
        stats[0] = R.launches;
        stats[1] = R.retries;
        stats[2] = R.compactions;
        stats[3] = R.appended;
        stats[4] = R.swept;
        stats[5] = R.skipped;
    }
    if (kernel_ms) *kernel_ms = ms;
    return GG_OK;
}
