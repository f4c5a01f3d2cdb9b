// set_sweep.h -- the parts the graph-only sweeps over the SET adjacency (gg::SetGraph, ensure_set_adjacency) share, written once
// for their users: pair_neighbors.hip (link indices), graph_prop.hip (neighbour sum, label spreading), communities.hip (neighbour
// mode, label propagation, partition edges), two_hop.hip (two-hop top-K and rank) and ppr_push.hip (rooted PageRank by local push);
// spanning_forest.hip takes the hash.  The consumers of a filled table that two_hop.hip and ppr_push.hip share: set_consume.h.
// Device part: the open-addressing (id, integer value) table of the hash-accumulate sweeps and the lower-bound search of the
// walk-the-shorter-list sweeps -- __forceinline__ throughout and integer only.  Host part: the task planner and the launcher of
// the three group widths, and the argument checks with the texts the entry points share.
#pragma once
#include <algorithm>
#include <vector>

#include "gg_internal.h"

namespace gg {

// The MurmurHash3 finaliser: the hash of the neighbour-mode ties and the label-propagation sides (communities.hip) and of the
// default edge priorities of the spanning forest (spanning_forest.hip).
__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}

// Slots of a table that takes `entries` distinct ids: the smallest power of two >= max(256, 2 entries), so that a probe always
// meets a free or a matching slot.
template <class I>
__host__ __device__ __forceinline__ I set_table_slots(I entries) {
    I T = 256;
    while (T < 2 * entries) T <<= 1;
    return T;
}

// An open-addressing table of (id + 1, V value) slots, 0 marking an empty slot, linear probing from id mod slots; V is uint32_t or
// unsigned long long.  GLOBAL: key and val lie in global memory zeroed by the host and are read back with relaxed agent-scope
// loads; else in LDS arrays the kernel declares, zeroed by clear_lds.  A workgroup fills the table with add, calls fill_done and
// then only reads it (find, ld_key / ld_val per slot) or clears values of its own slots (clear_val).
template <class V, bool GLOBAL>
struct SetTable {
    uint32_t *key;
    V *val;
    uint32_t mask;  // slots - 1
    // every thread of the 256-thread workgroup calls it, before the first add
    __device__ __forceinline__ void clear_lds() const {
        for (uint32_t s = threadIdx.x; s < mask + 1u; s += 256) key[s] = 0u, val[s] = (V)0;
        __syncthreads();
    }
    // the hand-over from the fill to the scan; every thread of the workgroup calls it
    __device__ __forceinline__ void fill_done() const {
        if (GLOBAL) __threadfence();
        __syncthreads();
    }
    __device__ __forceinline__ uint32_t ld_key(uint32_t s) const { return GLOBAL ? __hip_atomic_load(key + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : key[s]; }
    __device__ __forceinline__ V ld_val(uint32_t s) const { return GLOBAL ? __hip_atomic_load(val + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : val[s]; }
    __device__ __forceinline__ void clear_val(uint32_t s) const {
        if (GLOBAL) __hip_atomic_store(val + s, (V)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else val[s] = (V)0;
    }
    // the slot of id, claimed by compare-and-swap where no thread has claimed it yet
    __device__ __forceinline__ uint32_t claim(int id) const {
        const uint32_t k = (uint32_t)id + 1u;
        uint32_t s = (uint32_t)id & mask;
        for (;;) {
            const uint32_t old = atomicCAS(key + s, 0u, k);
            if (old == 0u || old == k) break;
            s = (s + 1u) & mask;
        }
        return s;
    }
    // value[id] += v: the slot is claimed, the value added with an integer atomic
    __device__ __forceinline__ void add(int id, V v) const { atomicAdd(val + claim(id), v); }
    // the value under id, 0 where no add named it (behind fill_done)
    __device__ __forceinline__ V find(int id) const {
        const uint32_t k = (uint32_t)id + 1u;
        uint32_t s = (uint32_t)id & mask;
        for (;;) {
            const uint32_t kk = ld_key(s);
            if (kk == 0u) return (V)0;
            if (kk == k) return ld_val(s);
            s = (s + 1u) & mask;
        }
    }
};

// The first position p in [lo, len) of the sorted list A with A[p] >= x (len if there is none).  A caller whose x ascend passes its
// last result as lo; x is in the list iff p < len && A[p] == x.
__device__ __forceinline__ int set_lower_bound(const int32_t *A, int lo, int len, int x) {
    int hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (A[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The tasks of n_item lists for the three group widths: a list of s = len_of(item) entries belongs to class 0 (s <= upto[0]: 4
// lanes), 1 (s <= upto[1]: 16 lanes) or 2 (64 lanes) and is cut into the tasks (item, c0), c0 = 0, chunk, 2 chunk, ... < s; an empty
// list gets the task (item, 0) if empty_task (the task stores the item's outputs), else none.  task holds the classes one behind
// the other, class c in [first[c], first[c + 1]), items and chunks ascending.  False: more than 2^31 - 1 tasks.
template <class LenOf>
bool plan_width_tasks(int n_item, LenOf len_of, const int (&upto)[2], int chunk, bool empty_task, std::vector<int2> &task, int64_t (&first)[4]) {
    const auto cls = [&](int64_t s) { return s <= upto[0] ? 0 : s <= upto[1] ? 1 : 2; };
    std::fill(first, first + 4, 0);
    for (int i = 0; i < n_item; ++i) {
        const int64_t s = len_of(i);
        first[cls(s) + 1] += s ? (s + chunk - 1) / chunk : empty_task;
    }
    for (int c = 0; c < 3; ++c) first[c + 1] += first[c];
    if (first[3] > 0x7fffffffLL) return false;
    task.resize((size_t)first[3]);
    int64_t fill[3] = {first[0], first[1], first[2]};
    for (int i = 0; i < n_item; ++i) {
        const int64_t s = len_of(i);
        int64_t &at = fill[cls(s)];
        if (s == 0 && empty_task) task[(size_t)at++] = make_int2(i, 0);
        for (int64_t c0 = 0; c0 < s; c0 += chunk) task[(size_t)at++] = make_int2(i, (int)c0);
    }
    return true;
}

// One launch per non-empty width class of a task list ordered like plan_width_tasks': groups of W = 4, 16, 64 lanes, 256 threads, at
// most max_blocks workgroups whose groups stride over the tasks behind them.  The three instantiations of the kernel are arguments
// (the call site names them); o.task / o.n_task are set per class.
template <class Args, class Task>
void launch_width_classes(hipStream_t stream, int max_blocks, const Task *task, const int64_t *first, Args o, void (*k4)(Args), void (*k16)(Args),
                          void (*k64)(Args)) {
    void (*const kernel[3])(Args) = {k4, k16, k64};
    for (int c = 0, W = 4; c < 3; ++c, W *= 4) {
        const int64_t n_task = first[c + 1] - first[c];
        if (n_task == 0) continue;
        o.task = task + first[c];
        o.n_task = (int)n_task;
        hipLaunchKernelGGL(kernel[c], dim3(std::min(max_blocks, cdiv(n_task, 256 / W))), dim3(256), 0, stream, o);
    }
}

// every ids[i] in [0, n_node), or the call fails naming the first that is not
inline int check_ids(gg_ctx *ctx, const char *fn, const char *name, const int32_t *ids, int64_t m) {
    const int n = ctx->n_node;
    for (int64_t i = 0; i < m; ++i)
        GG_CHECK(ctx, ids[i] >= 0 && ids[i] < n, GG_EINVAL, "%s: %s[%lld] = %d out of range [0, %d)", fn, name, (long long)i, ids[i], n);
    return GG_OK;
}

// the argument checks the entry points of the per-query sweeps (two_hop.hip, ppr_push.hip) share, in the order the header lists
// their texts; m_name: "n_rows" or "m"
inline int check_query_request(gg_ctx *ctx, const char *fn, int64_t m, const char *m_name, int exclude, int64_t scratch_bytes) {
    GG_CHECK(ctx, ctx->g_rowptr, GG_EINVAL, "%s: needs the training graph (gg_set_graph_csr)", fn);
    GG_CHECK(ctx, m >= 0, GG_EINVAL, "%s: %s = %lld is negative", fn, m_name, (long long)m);
    GG_CHECK(ctx, m <= 0x7fffffffLL, GG_EINVAL, "%s: %s = %lld does not fit in 31 bits", fn, m_name, (long long)m);
    GG_CHECK(ctx, exclude == 1 || exclude == 2, GG_EINVAL, "%s: exclude = %d is neither 1 (self) nor 2 (graph)", fn, exclude);
    GG_CHECK(ctx, scratch_bytes >= 0, GG_EINVAL, "%s: scratch_bytes = %lld is negative", fn, (long long)scratch_bytes);
    return GG_OK;
}

// A sum of per-node weights over a set of neighbours has at most max(deg) terms: it must stay below 2^63 (behind
// ensure_set_adjacency).
inline int check_weight_bound(gg_ctx *ctx, const char *fn, const uint64_t *weights, int64_t count) {
    uint64_t max_w = 0;
    for (int64_t k = 0; k < count; ++k) max_w = std::max(max_w, weights[k]);
    const int32_t deg = ctx->set.max_deg;
    GG_CHECK(ctx, max_w == 0 || deg == 0 || max_w <= 0x7fffffffffffffffull / (uint64_t)deg, GG_EINVAL,
             "%s: the largest weight %llu times the largest degree %d does not fit in 63 bits", fn, (unsigned long long)max_w, deg);
    return GG_OK;
}

}  // namespace gg
