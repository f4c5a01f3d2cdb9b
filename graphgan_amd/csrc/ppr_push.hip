// ppr_push.hip -- the push sweep behind the rooted-PageRank ranking baseline: per query node u the approximate personalised PageRank
// vector p of u on the resident training graph by the synchronous local push of Andersen, Chung & Lang in fixed-point integers
// (include/graphgan_hip.h, "push sweep": the rule, ONE = 2^40), and from it either the best k candidates (gg_ppr_topk) or the
// integers that place one target in the total order (gg_ppr_rank).  No embedding table is read: integer gathers over the SET
// adjacency of ensure_set_adjacency (pair_neighbors.hip).  The kernels hold no floating-point operation.
//
// Shape (the first build; what was not tuned is listed in DESIGN.md "Push sweep").  One workgroup of 256 threads per task; a task
// is one root -- for the rank, the run of adjacent queries with that root.  Per task one key array and two value arrays (r, p)
// over the same slots of an open-addressing SetTable (set_sweep.h), the frontier (two lists of slots that take turns), the share
// of every frontier entry and the list of the frontier's long lists.
//   table size  Every push of x retires keep >= deg(x) kmin, kmin = (eps_q alpha_q) >> 16 >= 1, and the retired mass never exceeds
//               ONE: the sum of deg(x) over all pushes of a query is at most B = ONE / kmin.  A node other than the root is touched
//               only as an entry of a pushed list, so at most E = min(n_node, 1 + B) distinct nodes ever get a slot.  The host
//               sizes the table with set_table_slots(E) >= 2 E slots: a probe always meets a free or a matching slot, and claim()
//               ends.  (A table that could fill would spin forever.)  The frontier holds distinct nodes: E entries suffice.
//               E <= PPR_LDS_CAP = 1024: everything lies in LDS (2048 slots x 20 B, 20 B per frontier entry, with the consumer's
//               buffers below 64 KiB); above, in zeroed global scratch (per task r, p, the keys, then the frontier), the tasks
//               batched under scratch_bytes.
//   phase A     one thread per frontier entry x: keep / share / rem from r0 = r[x]; p[x] += keep, r[x] = rem, the share is kept
//               beside the entry; an entry with more than PP_NARROW = 64 neighbours is noted in the list of long lists.
//   phase B     behind a barrier (global tables: the fence of fill_done).  Lists N(x) of up to 64 entries are walked by groups of
//               16 lanes, the noted long ones by all 256 lanes: no lane walks a hub alone.  r[w] += share is the table's claim
//               followed by a 64-bit integer atomic add that returns the old value.  At the start of phase B every r lies below
//               its threshold thr(w) = eps_q deg(w) (a pushed node is left with rem < deg, every other node was inactive), and
//               values only grow: exactly one adder sees old < thr(w) <= old + share and appends w to the next frontier.
//   rounds      the counters live in LDS and take turns with the round's parity, so a round costs two barriers; nothing crosses
//               to the host.  sum p is the sum of every keep: each thread sums its own, and residual = ONE - sum p is folded once.
//   consumers   set_rank_consume / set_topk_consume (set_consume.h, the two-hop sweep's) on (key, p).
// Every add is an integer and the pushes of a round read start-of-round values only, so a query's outputs depend on the graph,
// the parameters and the root alone -- not on the request, the grid, the batches, the order of the atomics or the run.
#include <algorithm>
#include <type_traits>

#include "set_consume.h"

namespace gg {

namespace {

constexpr int PPR_LDS_CAP = 1024;     // touched nodes E the LDS tables take (Engine.PPR_LDS_CAP); larger tasks use global memory
constexpr int PPR_LDS_SLOTS = 2 * PPR_LDS_CAP;
constexpr int PP_NARROW = 64;         // a list N(x) up to this length is walked by a 16-lane group, a longer one by the workgroup
constexpr int PP_BLOCKS = 2048;       // workgroups per launch at most; they stride over the tasks behind them
constexpr int64_t PP_SCRATCH = 2048ll << 20;  // default cap on the global tables of one pass, bytes
constexpr int64_t PP_CHUNK_OUT = 1ll << 23;   // list entries (queries x k) of one chunk of a top-K request at most
constexpr unsigned long long PP_ONE = 1ull << 40;
static_assert(PPR_LDS_SLOTS * (4 + 8 + 8) + PPR_LDS_CAP * (8 + 4 + 4 + 2) + 5 * 1024 <= 64 * 1024, "the LDS tables, the frontier and the consumer's buffers");

struct PpTask {
    int32_t q0, q1;   // queries [q0, q1) of the chunk: one root
    int64_t off;      // global tables: first 8-byte word of the task in tab
};

struct PpArgs {
    const PpTask *task;
    int n_task;
    unsigned long long *tab;          // zeroed global tables of the pass
    uint32_t slots;                   // table size of every task, a power of two
    uint32_t fcap;                    // frontier entries of every task (even)
    const int32_t *u, *v;             // [chunk] query nodes; targets (rank only)
    const int64_t *ptr;               // set adjacency
    const int32_t *adj;
    unsigned long long alpha_q, eps_q;
    int max_rounds;
    int excl;                         // 1: c != u; 2: c outside N(u) + {u}
    int k;
    int32_t *out_col;                 // top-K: [chunk, k]
    unsigned long long *out_score;    //        [chunk, k]
    int32_t *n_pos;                   // [chunk]
    unsigned long long *score;        // rank: [chunk]
    int32_t *ahead, *pos_below;       //       [chunk]
    int32_t *rounds, *converged;      // [chunk]
    unsigned long long *residual;     // [chunk]
};

template <bool GLOBAL>
using PpTab = SetTable<unsigned long long, GLOBAL>;

// 8-byte words of one task's global memory: r and p (slots each), the keys (slots / 2), the shares (fcap), the two frontier
// lists and the long-list indices (fcap / 2 each)
__host__ __device__ __forceinline__ int64_t pp_task_words(int64_t slots, int64_t fcap) { return 2 * slots + slots / 2 + fcap + 3 * (fcap / 2); }

template <bool GLOBAL>
struct PpState {
    using Wide = typename std::conditional<GLOBAL, uint32_t, uint16_t>::type;  // (index into the frontier: below PPR_LDS_CAP in LDS)
    PpTab<GLOBAL> r;            // (key, r)
    unsigned long long *p;      // over the same slots
    unsigned long long *sh;     // [fcap] the share of frontier entry i
    uint32_t *fr;               // [2, fcap] the frontier lists (slots)
    Wide *wide;                 // [fcap] the frontier entries with a long list
    uint32_t *cnt;              // LDS: next-frontier lengths [2], long-list counts [2], by round parity
    uint32_t fcap;
};

// the task's arrays: in LDS (declared here, cleared) or in the zeroed global tables.  Every thread of the workgroup calls it.
template <bool GLOBAL>
__device__ __forceinline__ PpState<GLOBAL> pp_state(const PpArgs &o, const PpTask &tk) {
    __shared__ uint32_t s_key[GLOBAL ? 1 : PPR_LDS_SLOTS];
    __shared__ unsigned long long s_r[GLOBAL ? 1 : PPR_LDS_SLOTS], s_p[GLOBAL ? 1 : PPR_LDS_SLOTS], s_sh[GLOBAL ? 1 : PPR_LDS_CAP];
    __shared__ uint32_t s_fr[GLOBAL ? 1 : 2 * PPR_LDS_CAP], s_cnt[4];
    __shared__ typename PpState<GLOBAL>::Wide s_wide[GLOBAL ? 1 : PPR_LDS_CAP];
    PpState<GLOBAL> st;
    st.cnt = s_cnt;
    st.r.mask = o.slots - 1u;
    if (GLOBAL) {
        unsigned long long *base = o.tab + tk.off;
        st.fcap = o.fcap;
        st.r.val = base;
        st.p = base + o.slots;
        st.r.key = (uint32_t *)(base + 2 * (int64_t)o.slots);
        st.sh = base + 2 * (int64_t)o.slots + o.slots / 2;
        st.fr = (uint32_t *)(st.sh + o.fcap);
        st.wide = (typename PpState<GLOBAL>::Wide *)(st.fr + 2 * (int64_t)o.fcap);
    } else {
        st.fcap = PPR_LDS_CAP;
        st.r.val = s_r;
        st.p = s_p;
        st.r.key = s_key;
        st.sh = s_sh;
        st.fr = s_fr;
        st.wide = s_wide;
        for (uint32_t s = threadIdx.x; s < o.slots; s += 256) s_key[s] = 0u, s_r[s] = 0ull, s_p[s] = 0ull;
        __syncthreads();
    }
    return st;
}

// r[w] += share; the adder that lifts r[w] over its threshold appends w's slot to the next frontier
template <bool GLOBAL>
__device__ __forceinline__ void pp_add(const PpArgs &o, const PpState<GLOBAL> &st, int w, unsigned long long share, uint32_t *next, uint32_t *n_next) {
    const uint32_t s = st.r.claim(w);
    const unsigned long long old = atomicAdd(st.r.val + s, share);
    const unsigned long long thr = o.eps_q * (unsigned long long)(o.ptr[w + 1] - o.ptr[w]);  // (w is somebody's neighbour: deg(w) >= 1)
    if (old < thr && old + share >= thr) {
        const uint32_t j = atomicAdd(n_next, 1u);
        if (j < st.fcap) next[j] = s;  // (j < E <= fcap: the frontier holds distinct touched nodes)
    }
}

// The rounds of root u.  Every thread of the workgroup calls it (barriers inside) and returns the same rounds, converged and
// residual; behind it (key, p) is ready for the consumers.
template <bool GLOBAL>
__device__ __forceinline__ void pp_solve(const PpArgs &o, const PpState<GLOBAL> &st, int u, int &rounds, int &converged, unsigned long long &residual) {
    __shared__ unsigned long long r_keep[4];
    const int tid = threadIdx.x, gl = tid & 15;
    if (tid == 0) {
        const uint32_t s = st.r.claim(u);
        if (GLOBAL) __hip_atomic_store(st.r.val + s, PP_ONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else st.r.val[s] = PP_ONE;
        const unsigned long long du = (unsigned long long)(o.ptr[u + 1] - o.ptr[u]);
        const bool active = PP_ONE >= o.eps_q * (du ? du : 1ull);
        if (active) st.fr[st.fcap] = s;
        st.cnt[0] = 0u, st.cnt[1] = active, st.cnt[2] = 0u, st.cnt[3] = 0u;
    }
    st.r.fill_done();
    unsigned long long kept = 0ull;
    uint32_t nf = st.cnt[1];
    for (rounds = 0; nf > 0u && rounds < o.max_rounds; ++rounds) {  // (block-uniform: the barriers below are reached by every thread)
        const int par = rounds & 1;
        const uint32_t *cur = st.fr + (par ? 0u : st.fcap);
        uint32_t *next = st.fr + (par ? st.fcap : 0u);
        if (tid == 0) st.cnt[par] = 0u;  // (last read behind the round before the last; first added to behind this phase's barrier)
        for (uint32_t i = tid; i < nf; i += 256) {
            const uint32_t s = cur[i];
            const int x = (int)(st.r.ld_key(s) - 1u);
            const unsigned long long r0 = st.r.ld_val(s);
            const unsigned long long deg = (unsigned long long)(o.ptr[x + 1] - o.ptr[x]);
            const unsigned long long keep = deg ? (r0 * o.alpha_q) >> 16 : r0;
            const unsigned long long rest = r0 - keep;
            const unsigned long long share = deg ? rest / deg : 0ull;
            const unsigned long long rem = rest - share * deg;
            if (GLOBAL) {
                atomicAdd(st.p + s, keep);
                __hip_atomic_store(st.r.val + s, rem, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                st.p[s] += keep;
                st.r.val[s] = rem;
            }
            st.sh[i] = share;
            kept += keep;
            if (deg > (unsigned long long)PP_NARROW) {
                const uint32_t j = atomicAdd(&st.cnt[2 + par], 1u);
                if (j < st.fcap) st.wide[j] = (typename PpState<GLOBAL>::Wide)i;
            }
        }
        st.r.fill_done();
        if (tid == 0) st.cnt[2 + (par ^ 1)] = 0u;  // (last read in phase B of the round before; first added to in the next phase A)
        for (uint32_t i = tid >> 4; i < nf; i += 16) {
            const int x = (int)(st.r.ld_key(cur[i]) - 1u);
            const int64_t xb = o.ptr[x];
            const int deg = (int)(o.ptr[x + 1] - xb);
            if (deg > PP_NARROW) continue;
            const unsigned long long share = st.sh[i];
            for (int e = gl; e < deg; e += 16) pp_add<GLOBAL>(o, st, o.adj[xb + e], share, next, &st.cnt[par]);
        }
        const uint32_t nw = min(st.cnt[2 + par], st.fcap);
        for (uint32_t j = 0; j < nw; ++j) {
            const uint32_t i = st.wide[j];
            const int x = (int)(st.r.ld_key(cur[i]) - 1u);
            const int64_t xb = o.ptr[x];
            const int deg = (int)(o.ptr[x + 1] - xb);
            const unsigned long long share = st.sh[i];
            for (int e = tid; e < deg; e += 256) pp_add<GLOBAL>(o, st, o.adj[xb + e], share, next, &st.cnt[par]);
        }
        st.r.fill_done();
        nf = min(st.cnt[par], st.fcap);
    }
    converged = nf == 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) kept += (unsigned long long)__shfl_xor(kept, off, 64);
    if ((tid & 63) == 0) r_keep[tid >> 6] = kept;
    __syncthreads();
    residual = PP_ONE - (r_keep[0] + r_keep[1] + r_keep[2] + r_keep[3]);
}

template <bool GLOBAL>
__global__ __launch_bounds__(256) void pp_rank_kernel(PpArgs o) {
    const int tid = threadIdx.x;
    for (int t = blockIdx.x; t < o.n_task; t += gridDim.x) {  // (block-uniform: the barriers below are reached by every thread)
        const PpTask tk = o.task[t];
        const int u = o.u[tk.q0];
        const PpState<GLOBAL> st = pp_state<GLOBAL>(o, tk);
        int rounds, converged;
        unsigned long long residual;
        pp_solve<GLOBAL>(o, st, u, rounds, converged, residual);
        PpTab<GLOBAL> tb;
        tb.key = st.r.key, tb.val = st.p, tb.mask = st.r.mask;
        const int64_t ub = o.ptr[u];
        const int du = (int)(o.ptr[u + 1] - ub);
        for (int i = tk.q0; i < tk.q1; ++i) {  // one scan per target of the run
            const int v = o.v[i];
            unsigned long long sv;
            int np, ah, below;
            set_rank_consume<GLOBAL>(tb, o.slots, u, v, o.adj + ub, du, o.excl, sv, np, ah, below);
            if (tid == 0) {
                o.score[i] = sv;
                o.n_pos[i] = np;
                o.ahead[i] = ah;
                o.pos_below[i] = below;
                o.rounds[i] = rounds;
                o.converged[i] = converged;
                o.residual[i] = residual;
            }
            __syncthreads();  // (the next scan, or the next task, reuses the fold words and the tables)
        }
    }
}

template <bool GLOBAL>
__global__ __launch_bounds__(256) void pp_topk_kernel(PpArgs o) {
    const int tid = threadIdx.x;
    for (int t = blockIdx.x; t < o.n_task; t += gridDim.x) {  // (block-uniform: the barriers below are reached by every thread)
        const PpTask tk = o.task[t];
        const int i = tk.q0, u = o.u[i];
        const PpState<GLOBAL> st = pp_state<GLOBAL>(o, tk);
        int rounds, converged;
        unsigned long long residual;
        pp_solve<GLOBAL>(o, st, u, rounds, converged, residual);
        PpTab<GLOBAL> tb;
        tb.key = st.r.key, tb.val = st.p, tb.mask = st.r.mask;
        const int64_t ub = o.ptr[u];
        const int du = (int)(o.ptr[u + 1] - ub);
        set_topk_consume<GLOBAL>(tb, o.slots, u, o.adj + ub, du, o.excl, o.k, (int64_t)i, o.out_col, o.out_score, o.n_pos);
        if (tid == 0) {
            o.rounds[i] = rounds;
            o.converged[i] = converged;
            o.residual[i] = residual;
        }
        __syncthreads();  // (the next task clears the tables, the list and the fold words)
    }
}

// The sweep of one request: `rank` selects the outputs.  Queries go in chunks (bounded device memory for the outputs).  Every task
// of a request has the same table size (E depends on the parameters and n_node alone): either all tables lie in LDS and a chunk is
// one launch, or all lie in global memory and a chunk takes as many passes as scratch_bytes asks for (a pass takes at least one
// task, whatever its size).
int pp_run(gg_ctx *ctx, const char *fn, bool rank, const int32_t *u, const int32_t *v, int64_t m, int k, uint32_t alpha_q, uint64_t eps_q, int max_rounds, int excl,
           int64_t scratch_bytes, int32_t *out_col, uint64_t *out_score, uint64_t *score, int32_t *ahead, int32_t *n_pos, int32_t *pos_below, int32_t *rounds,
           int32_t *converged, uint64_t *residual, double *kernel_ms) {
    const int n = ctx->n_node;
    GG_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = ensure_set_adjacency(ctx);
    if (rc != GG_OK) return rc;
    const int64_t cap = scratch_bytes > 0 ? scratch_bytes : PP_SCRATCH;
    const uint64_t kmin = (eps_q * alpha_q) >> 16;  // (>= 1: checked by the entry points)
    const int64_t E = std::min<int64_t>(n, 1 + (int64_t)(PP_ONE / kmin));
    const bool lds = E <= PPR_LDS_CAP;
    const int64_t slots = set_table_slots(E), fcap = lds ? PPR_LDS_CAP : (E + 1) / 2 * 2;
    const int64_t words = pp_task_words(slots, fcap);
    const int64_t per_pass = lds ? 0 : std::max<int64_t>(1, cap / (words * 8));
    const int64_t chunk = rank ? std::min<int64_t>(m, 1 << 20) : std::min<int64_t>(m, std::max<int64_t>(1, PP_CHUNK_OUT / k));
    ScopedBuf d_u, d_v, d_task, d_col, d_sc, d_np, d_ah, d_below, d_rounds, d_conv, d_res;
    hipError_t e = d_u.reserve(sizeof(int32_t) * (size_t)chunk);
    for (ScopedBuf *b : {&d_np, &d_rounds, &d_conv})
        if (e == hipSuccess) e = b->reserve(sizeof(int32_t) * (size_t)chunk);
    if (e == hipSuccess) e = d_res.reserve(sizeof(uint64_t) * (size_t)chunk);
    if (e == hipSuccess) e = d_task.reserve(sizeof(PpTask) * (size_t)chunk);
    if (rank) {
        for (ScopedBuf *b : {&d_v, &d_ah, &d_below})
            if (e == hipSuccess) e = b->reserve(sizeof(int32_t) * (size_t)chunk);
        if (e == hipSuccess) e = d_sc.reserve(sizeof(uint64_t) * (size_t)chunk);
    } else {
        if (e == hipSuccess) e = d_col.reserve(sizeof(int32_t) * (size_t)chunk * k);
        if (e == hipSuccess) e = d_sc.reserve(sizeof(uint64_t) * (size_t)chunk * k);
    }
    if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "%s: %s", fn, hipGetErrorString(e));
    std::vector<PpTask> task;
    double ms_total = 0.0;
    for (int64_t p0 = 0; p0 < m; p0 += chunk) {
        const int cr = (int)std::min<int64_t>(chunk, m - p0);
        // the chunk's tasks: for the rank one per run of adjacent queries with the same root, else one per query
        task.clear();
        for (int i = 0; i < cr;) {
            int j = i + 1;
            while (rank && j < cr && u[p0 + j] == u[p0 + i]) ++j;
            PpTask tk;
            tk.q0 = i, tk.q1 = j;
            tk.off = lds ? 0 : (int64_t)(task.size() % (size_t)per_pass) * words;
            task.push_back(tk);
            i = j;
        }
        const int64_t n_task = (int64_t)task.size();
        const int64_t pass_tasks = lds ? n_task : std::min(per_pass, n_task);
        if (!lds) {
            e = ctx->set.th_tab.reserve(sizeof(uint64_t) * (size_t)(pass_tasks * words));
            if (e != hipSuccess) return fail(ctx, GG_ENOMEM, "%s: %lld bytes of table scratch: %s", fn, (long long)(pass_tasks * words * 8), hipGetErrorString(e));
        }
        GG_HIP_FN(hipMemcpyAsync(d_u.p, u + p0, sizeof(int32_t) * cr, hipMemcpyHostToDevice, ctx->stream));
        if (rank) GG_HIP_FN(hipMemcpyAsync(d_v.p, v + p0, sizeof(int32_t) * cr, hipMemcpyHostToDevice, ctx->stream));
        GG_HIP_FN(hipMemcpyAsync(d_task.p, task.data(), sizeof(PpTask) * (size_t)n_task, hipMemcpyHostToDevice, ctx->stream));
        PpArgs o{};
        o.tab = ctx->set.th_tab.as<unsigned long long>();
        o.slots = (uint32_t)slots;
        o.fcap = (uint32_t)fcap;
        o.u = d_u.as<int32_t>();
        o.v = d_v.as<int32_t>();
        o.ptr = ctx->set.ptr.as<int64_t>();
        o.adj = ctx->set.adj.as<int32_t>();
        o.alpha_q = alpha_q;
        o.eps_q = eps_q;
        o.max_rounds = max_rounds;
        o.excl = excl;
        o.k = k;
        o.out_col = d_col.as<int32_t>();
        o.out_score = rank ? nullptr : d_sc.as<unsigned long long>();
        o.score = rank ? d_sc.as<unsigned long long>() : nullptr;
        o.n_pos = d_np.as<int32_t>();
        o.ahead = d_ah.as<int32_t>();
        o.pos_below = d_below.as<int32_t>();
        o.rounds = d_rounds.as<int32_t>();
        o.converged = d_conv.as<int32_t>();
        o.residual = d_res.as<unsigned long long>();
        (void)hipEventRecord(ctx->ev0, ctx->stream);
        for (int64_t t0 = 0; t0 < n_task; t0 += pass_tasks) {
            const int64_t nt = std::min(pass_tasks, n_task - t0);
            o.task = d_task.as<PpTask>() + t0;
            o.n_task = (int)nt;
            const dim3 grid((unsigned)std::min<int64_t>(PP_BLOCKS, nt));
            if (lds) {
                if (rank) hipLaunchKernelGGL(pp_rank_kernel<false>, grid, dim3(256), 0, ctx->stream, o);
                else hipLaunchKernelGGL(pp_topk_kernel<false>, grid, dim3(256), 0, ctx->stream, o);
            } else {
                GG_HIP_FN(hipMemsetAsync(ctx->set.th_tab.p, 0, sizeof(uint64_t) * (size_t)(nt * words), ctx->stream));
                if (rank) hipLaunchKernelGGL(pp_rank_kernel<true>, grid, dim3(256), 0, ctx->stream, o);
                else hipLaunchKernelGGL(pp_topk_kernel<true>, grid, dim3(256), 0, ctx->stream, o);
            }
        }
        (void)hipEventRecord(ctx->ev1, ctx->stream);
        GG_HIP_FN(hipGetLastError());
        GG_HIP_FN(hipMemcpyAsync(n_pos + p0, d_np.p, sizeof(int32_t) * cr, hipMemcpyDeviceToHost, ctx->stream));
        GG_HIP_FN(hipMemcpyAsync(rounds + p0, d_rounds.p, sizeof(int32_t) * cr, hipMemcpyDeviceToHost, ctx->stream));
        GG_HIP_FN(hipMemcpyAsync(converged + p0, d_conv.p, sizeof(int32_t) * cr, hipMemcpyDeviceToHost, ctx->stream));
        GG_HIP_FN(hipMemcpyAsync(residual + p0, d_res.p, sizeof(uint64_t) * cr, hipMemcpyDeviceToHost, ctx->stream));
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

// the parameter ranges of the rule, in the order the header lists their texts
int pp_check(gg_ctx *ctx, const char *fn, uint32_t alpha_q, uint64_t eps_q, int max_rounds) {
    GG_CHECK(ctx, alpha_q >= 1u && alpha_q <= 65535u, GG_EINVAL, "%s: alpha_q = %u outside [1, 65535]", fn, alpha_q);
    GG_CHECK(ctx, eps_q >= 1ull && eps_q <= (1ull << 32), GG_EINVAL, "%s: eps_q = %llu outside [1, 4294967296]", fn, (unsigned long long)eps_q);
    GG_CHECK(ctx, max_rounds >= 1, GG_EINVAL, "%s: max_rounds = %d is below 1", fn, max_rounds);
    GG_CHECK(ctx, (uint64_t)alpha_q * eps_q >= 65536ull, GG_EINVAL, "%s: alpha_q * eps_q = %llu is below 65536 (alpha_q = %u, eps_q = %llu)", fn,
             (unsigned long long)(alpha_q * eps_q), alpha_q, (unsigned long long)eps_q);
    return GG_OK;
}

}  // namespace

}  // namespace gg

using namespace gg;

// gg_ppr_topk, gg_ppr_rank: see include/graphgan_hip.h.
extern "C" int gg_ppr_topk(gg_ctx *ctx, const int32_t *rows, int64_t n_rows, int32_t k, uint32_t alpha_q, uint64_t eps_q, int32_t max_rounds, int32_t exclude,
                           int64_t scratch_bytes, int32_t *out_col, uint64_t *out_score, int32_t *n_pos, int32_t *rounds, int32_t *converged, uint64_t *residual,
                           double *kernel_ms) {
    const char *fn = "gg_ppr_topk";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (kernel_ms) *kernel_ms = 0.0;
    int rc = check_query_request(ctx, fn, n_rows, "n_rows", exclude, scratch_bytes);
    if (rc != GG_OK) return rc;
    GG_CHECK(ctx, k >= 1 && k <= SET_MAX_K, GG_EINVAL, "%s: k = %d outside [1, %d]", fn, k, SET_MAX_K);
    rc = pp_check(ctx, fn, alpha_q, eps_q, max_rounds);
    if (rc != GG_OK) return rc;
    if (n_rows == 0) return GG_OK;
    GG_CHECK(ctx, rows && out_col && out_score && n_pos && rounds && converged && residual, GG_EINVAL,
             "%s: rows, out_col, out_score, n_pos, rounds, converged and residual must not be NULL", fn);
    rc = check_ids(ctx, fn, "rows", rows, n_rows);
    if (rc != GG_OK) return rc;
    return pp_run(ctx, fn, false, rows, nullptr, n_rows, k, alpha_q, eps_q, max_rounds, exclude, scratch_bytes, out_col, out_score, nullptr, nullptr, n_pos, nullptr,
                  rounds, converged, residual, kernel_ms);
}

extern "C" int gg_ppr_rank(gg_ctx *ctx, const int32_t *u, const int32_t *v, int64_t m, uint32_t alpha_q, uint64_t eps_q, int32_t max_rounds, int32_t exclude,
                           int64_t scratch_bytes, uint64_t *score, int32_t *ahead, int32_t *n_pos, int32_t *pos_below, int32_t *rounds, int32_t *converged,
                           uint64_t *residual, double *kernel_ms) {
    const char *fn = "gg_ppr_rank";
    if (!ctx) return fail(nullptr, GG_EINVAL, "ctx is NULL");
    if (kernel_ms) *kernel_ms = 0.0;
    int rc = check_query_request(ctx, fn, m, "m", exclude, scratch_bytes);
    if (rc == GG_OK) rc = pp_check(ctx, fn, alpha_q, eps_q, max_rounds);
    if (rc != GG_OK) return rc;
    if (m == 0) return GG_OK;
    GG_CHECK(ctx, u && v && score && ahead && n_pos && pos_below && rounds && converged && residual, GG_EINVAL,
             "%s: u, v, score, ahead, n_pos, pos_below, rounds, converged and residual must not be NULL", fn);
    rc = check_ids(ctx, fn, "u", u, m);
    if (rc == GG_OK) rc = check_ids(ctx, fn, "v", v, m);
    if (rc != GG_OK) return rc;
    return pp_run(ctx, fn, true, u, v, m, 1, alpha_q, eps_q, max_rounds, exclude, scratch_bytes, nullptr, nullptr, score, ahead, n_pos, pos_below, rounds, converged,
                  residual, kernel_ms);
}
