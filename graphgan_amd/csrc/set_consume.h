// set_consume.h -- the consumers of a filled (column, uint64 score) SetTable (set_sweep.h), written once for the sweeps that
// rank every node by an integer score of one query node u: two_hop.hip (the two-hop sweep), ppr_push.hip (the push sweep) and
// two_hop_pairs.hip (the two-hop pair sweep: the floor consumer).
// Device code only, __forceinline__ and integer only; each function declares the LDS it needs itself, so a kernel that inlines
// one gets exactly that consumer's buffers.  Every thread of the 256-thread workgroup calls them (barriers inside), behind the
// table's fill_done.
//   set_rank_consume   the target's slot is looked up, then the table is scanned once: eligibility is c != u, c != v plus, under
//                      excl = 2, a binary search in the sorted N(u); n_pos, ahead and pos_below are counted with compares, folded
//                      per wavefront by shuffles and per workgroup through LDS;
//   set_topk_consume   the scan zeroes the values of the ineligible entries in place and folds n_pos and the largest score; if
//                      n_pos > k a radix select on the composite key (score, ~column) -- 8 bits per pass from the first non-zero
//                      byte of the largest score down, an LDS histogram with integer adds, the bucket found by a workgroup scan --
//                      ends at the first byte whose bucket holds exactly the entries still wanted; the min(k, n_pos) survivors are
//                      gathered into LDS and bitonic-sorted (score descending, column ascending).  Composite keys are distinct, so
//                      selection and order are exact;
//   set_floor_consume  the table of source u is scanned once against ONE global floor (fs, fu, fv), the k-th best pair {u, v}, u < v,
//                      known to the whole run: an entry (c, x) survives when x > 0, c > u, c has its bit in the set's bitmap
//                      (instances with one), c is outside the sorted N(u) (exclude) and (x, u, c) is strictly ahead of the floor;
//                      the survivors are appended as (score lo, score hi, u, c) to a global buffer with ONE integer atomic per
//                      wavefront and scan step on the fill counter (ballot, popcount, prefix).  The counter keeps counting past
//                      the capacity, the stores do not.  It needs no LDS.
#pragma once
#include "set_sweep.h"

namespace gg {

constexpr int SET_MAX_K = 256;  // list length at most: the survivors are sorted by one workgroup of 256 threads

// x in the sorted list A[0, len)
__device__ __forceinline__ bool set_member(const int32_t *A, int len, int x) {
    const int p = set_lower_bound(A, 0, len, x);
    return p < len && A[p] == x;
}

// "a comes before b": score descending, column ascending
__device__ __forceinline__ bool set_before(unsigned long long sa, uint32_t ca, unsigned long long sb, uint32_t cb) {
    return sa > sb || (sa == sb && ca < cb);
}

// The integers that place target v of query u: sv = the value under v, and over the eligible c != v with a value > 0 np (all of
// them), ah (those before v in the order) and below (those with c < v); Nu / du: the sorted N(u).  All threads return the same four.
// The caller puts a barrier between its reads of the results and the next call (the fold words).
template <bool GLOBAL>
__device__ __forceinline__ void set_rank_consume(const SetTable<unsigned long long, GLOBAL> &tb, uint32_t slots, int u, int v, const int32_t *Nu, int du, int excl,
                                                 unsigned long long &sv, int &np, int &ah, int &below) {
    __shared__ int r_cnt[4][3];
    const int tid = threadIdx.x;
    sv = tb.find(v);  // (the same probes in every thread)
    np = 0, ah = 0, below = 0;
    for (uint32_t s = tid; s < slots; s += 256) {
        const uint32_t k = tb.ld_key(s);
        if (k == 0u) continue;
        const unsigned long long x = tb.ld_val(s);
        const int c = (int)(k - 1u);
        if (x == 0ull || c == u || c == v) continue;
        if (excl == 2 && set_member(Nu, du, c)) continue;
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
    np = r_cnt[0][0] + r_cnt[1][0] + r_cnt[2][0] + r_cnt[3][0];
    ah = r_cnt[0][1] + r_cnt[1][1] + r_cnt[2][1] + r_cnt[3][1];
    below = r_cnt[0][2] + r_cnt[1][2] + r_cnt[2][2] + r_cnt[3][2];
}

// The first k eligible entries with a value > 0 of query u in the order, into row i of out_col / out_score [., k] (padding: column
// -1, score 0), and their number into n_pos[i].  The values of the ineligible entries are zeroed in the table.  The caller puts a
// barrier between this call and the next use of the table or the next call.
template <bool GLOBAL>
__device__ __forceinline__ void set_topk_consume(const SetTable<unsigned long long, GLOBAL> &tb, uint32_t slots, int u, const int32_t *Nu, int du, int excl, int k_out,
                                                 int64_t i, int32_t *out_col, unsigned long long *out_score, int32_t *n_pos) {
    __shared__ unsigned long long s_sc[SET_MAX_K], r_max[4], s_thr_hi;
    __shared__ uint32_t s_cl[SET_MAX_K], s_hist[256], r_sum[4], s_thr_lo, s_rem, s_n, s_done;
    const int tid = threadIdx.x;
    // Every scan below gives slot s to thread s mod 256, so a thread reads back only the zeroes it stored itself.
    uint32_t np = 0;
    unsigned long long mx = 0ull;
    for (uint32_t s = tid; s < slots; s += 256) {
        const uint32_t k = tb.ld_key(s);
        if (k == 0u) continue;
        const unsigned long long x = tb.ld_val(s);
        if (x == 0ull) continue;
        const int c = (int)(k - 1u);
        if (c == u || (excl == 2 && set_member(Nu, du, c))) {
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
    if (tid == 0) s_thr_hi = 0ull, s_thr_lo = 0u, s_rem = (uint32_t)k_out, s_n = 0u, s_done = 0u;
    __syncthreads();
    np = r_sum[0] + r_sum[1] + r_sum[2] + r_sum[3];
    mx = max(max(r_max[0], r_max[1]), max(r_max[2], r_max[3]));
    if (np > (uint32_t)k_out) {  // (block-uniform) the k-th largest composite key, byte by byte from the top
        for (int b = 4 + (63 - __clzll((long long)mx)) / 8; b >= 0; --b) {  // (mx > 0; bytes above b are zero in every score)
            s_hist[tid] = 0u;
            __syncthreads();  // (also: the threshold words of the pass before)
            const unsigned long long thi = s_thr_hi;
            const uint32_t tlo = s_thr_lo, rem = s_rem;
            for (uint32_t s = tid; s < slots; s += 256) {
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
    for (uint32_t s = tid; s < slots; s += 256) {
        const uint32_t k = tb.ld_key(s);
        if (k == 0u) continue;
        const unsigned long long x = tb.ld_val(s);
        if (x == 0ull) continue;
        const uint32_t lo = ~(k - 1u);
        if (x > thi || (x == thi && lo >= tlo)) {
            const uint32_t p = atomicAdd(&s_n, 1u);
            if (p < (uint32_t)SET_MAX_K) s_sc[p] = x, s_cl[p] = k - 1u;  // (p < min(k, n_pos) by the selection)
        }
    }
    __syncthreads();
    for (int k2 = 2; k2 <= SET_MAX_K; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            const int p = tid ^ j;
            if (p > tid) {
                const bool up = (tid & k2) == 0;
                const unsigned long long sa = s_sc[tid], sb = s_sc[p];
                const uint32_t ca = s_cl[tid], cb = s_cl[p];
                if (set_before(sb, cb, sa, ca) == up) s_sc[tid] = sb, s_cl[tid] = cb, s_sc[p] = sa, s_cl[p] = ca;
            }
            __syncthreads();
        }
    if (tid < k_out) {
        out_col[i * k_out + tid] = (int32_t)s_cl[tid];
        out_score[i * k_out + tid] = s_sc[tid];
    }
    if (tid == 0) n_pos[i] = (int32_t)np;
}

// The floor of a pair sweep and where its survivors go.  The floor is the k-th best pair known, (0, max, max) -- "nothing is
// behind it": every score > 0 is ahead -- until k pairs are known; a kernel reads it once.
struct SetFloor {
    unsigned long long fs;
    int fu, fv;
    const uint32_t *member;  // [ceil(n_node / 32)] bit c: node c is in the set (instances with a bitmap)
    uint32_t *fill;          // entries appended so far (counts on past cap)
    uint32_t cap;
    uint4 *buf;              // [cap] (score lo, score hi, u, v)
};

// Every entry (c, x) of source u's table that is a candidate pair {u, c} strictly ahead of the floor, appended to f.buf.  Nu / du:
// the sorted N(u), searched under excl.  slots is a multiple of 256, so all 64 lanes of a wavefront take part in every ballot.
template <bool GLOBAL, bool BM>
__device__ __forceinline__ void set_floor_consume(const SetTable<unsigned long long, GLOBAL> &tb, uint32_t slots, int u, const int32_t *Nu, int du, int excl,
                                                  const SetFloor &f) {
    const int lane = threadIdx.x & 63;
    for (uint32_t s0 = 0; s0 < slots; s0 += 256) {
        const uint32_t s = s0 + threadIdx.x;
        const uint32_t k = tb.ld_key(s);
        unsigned long long x = 0ull;
        int c = 0;
        bool p = false;
        if (k != 0u) {
            x = tb.ld_val(s);
            c = (int)(k - 1u);
            p = x > 0ull && c > u && (x > f.fs || (x == f.fs && (u < f.fu || (u == f.fu && c < f.fv))));
            if (BM && p) p = ((f.member[c >> 5] >> (c & 31)) & 1u) != 0u;
            if (p && excl) p = !set_member(Nu, du, c);
        }
        const unsigned long long hit = __builtin_amdgcn_ballot_w64(p);
        if (hit == 0ull) continue;  // (wavefront-uniform)
        const uint32_t total = (uint32_t)__popcll(hit);
        const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(hit >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hit, 0u));
        uint32_t base = 0u;
        if (lane == 0) base = atomicAdd(f.fill, total);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        const uint32_t at = base + before;
        if (p && at < f.cap) f.buf[at] = make_uint4((uint32_t)x, (uint32_t)(x >> 32), (uint32_t)u, (uint32_t)c);
    }
}

}  // namespace gg
