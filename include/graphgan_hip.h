/*
 * graphgan_hip.h -- C ABI of libgraphgan_hip.so, the MI355X (gfx950) engine for the
 * GraphGAN hot path.  Plain C, no torch / numpy types: pointers, sizes, scalars.
 *
 * The reference (hwwang55/GraphGAN) has no FFI: its "operator API" is the five
 * tf.Session.run call sites of src/GraphGAN/graph_gan.py plus the host-side sampler.
 * Every entry point below names the reference interface it replaces (file:line under
 * /root/reference).  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - every function returns int: 0 = GG_OK, negative = GG_E*; no exceptions / aborts cross
 *     the ABI; gg_last_error() gives the message of the last failing call
 *     (ctx == NULL: the last gg_create / host-only failure of the calling thread).
 *   - the caller owns every host buffer it passes (C-contiguous; int32 node ids - the
 *     reference's placeholders are tf.int32, generator.py:17-18; fp32 values; int64
 *     offsets).  Inputs are copied; outputs are written before the call returns.  By default
 *     every call is synchronous (it returns after the context's HIP stream is idle).  The two
 *     exceptions are opt-in: after gg_set_profiling(ctx, k) with k != 1, gg_d_pass / gg_g_pass
 *     return once their kernels are ENQUEUED (stream-ordered behind everything issued before;
 *     they have no host outputs) -- errors of such a pass surface at the next call that
 *     synchronises (gg_prepare_*, gg_get_*, gg_synchronize); and gg_prepare_g_begin, which only
 *     enqueues the walks of the gg_prepare_g that follows (errors surface in that call).
 *   - a gg_ctx owns all device memory (embedding tables, Adam slots, graph CSR, tree CSR,
 *     prepared sample buffers, scratch) and one HIP stream on one device; it is not
 *     re-entrant.  Multi-GPU = one process and one context per GPU (gg_comm_*).
 *   - per-root outcomes (the reference's ``return None, None``) are DATA (root_status),
 *     not errors.
 *   - there is no CPU fallback: without a gfx950 device gg_create fails with GG_EHIP.
 */
#ifndef GRAPHGAN_HIP_H
#define GRAPHGAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GG_ABI_VERSION 9  /* (gg_pretrain_set_noise / gg_prepare_pretrain / gg_pretrain_set_walk_bias are ADDITIVE: new symbols, nothing existing changes, the number stays) gg_graph_softmax; 8: gg_topk_scores; round 6: lazy trees (gg_set_tree_mode, gg_lazy_stats, gg_get_lazy_trees); round 5: gg_comm_stats_ex; round 4: epoch over root batches (gg_epoch_*, gg_q3_*); round 3: gg_counters extended, gg_prepare_g_begin */

enum {
    GG_OK = 0,
    GG_EINVAL = -1,    /* bad argument / call order */
    GG_ECAPACITY = -2, /* caller capacity too small (e.g. path stride) */
    GG_EHIP = -3,      /* HIP runtime error, or no usable device */
    GG_ECOMM = -4,     /* RCCL error / librccl not loadable */
    GG_ENOMEM = -5,
    GG_EIO = -6
};

/* optimizer modes (a12) */
enum {
    GG_OPT_ADAM_DENSE = 0, /* TF1.8 sparse-apply semantics: m, v and var move over ALL rows each step */
    GG_OPT_ADAM_LAZY = 1,  /* only touched rows decay/move (scale mode) */
    GG_OPT_SGD = 2         /* var -= lr * grad on touched rows (north-star SGD variant) */
};

/* root_status values written by gg_walk_sample / gg_prepare_* */
enum {
    GG_ROOT_OK = 0,
    GG_ROOT_ABORTED = 1, /* reference: sample() returned (None, None), graph_gan.py:252-257 */
    GG_ROOT_EMPTY = 2    /* zero walks requested (D-mode, deg == 0): reference returns ([], []) */
};

/* hyper-parameters, names as in src/GraphGAN/config.py:4-25 */
typedef struct gg_config {
    float lr_gen;      /* config.py:9  */
    float lr_dis;      /* config.py:10 */
    float lambda_gen;  /* config.py:6  */
    float lambda_dis;  /* config.py:7  */
    float adam_beta1;  /* tf.train.AdamOptimizer default 0.9   */
    float adam_beta2;  /* 0.999 */
    float adam_eps;    /* 1e-8  */
    int32_t window_size; /* config.py:25.  >= 1: gg_create refuses anything below with GG_EINVAL.  No upper limit: a path of
                            L nodes has no pair further apart than L - 1, so every window from the longest path on gives the
                            same pairs (gg_prepare_g expands with min(window_size, path stride)) */
    int32_t optimizer;   /* GG_OPT_* */
    int32_t device;      /* HIP device ordinal */
    int32_t reserved[6];
} gg_config;

typedef struct gg_counters {
    int64_t walks;          /* walks completed since creation */
    int64_t hops;           /* sampled edges: one softmax-sample each (graph_gan.py:262-263) */
    int64_t nbr_reads;      /* sum over hops of k = tree neighbours scored */
    int64_t reward_pairs;   /* rows through gg_pair_reward / prepare_g */
    int64_t d_pairs;        /* rows through d steps */
    int64_t g_pairs;        /* rows through g steps */
    int64_t d_steps;
    int64_t g_steps;
    double last_kernel_ms;  /* HIP-event time of the last timed kernel region (walk / pass) */
    double walk_kernel_ms;  /* cumulative HIP-event time of the profiled gg_walk_sample / prepare walk launches */
    int64_t walk_launches;  /* ... and their number */
    int64_t rows_scored;    /* neighbour rows actually streamed: identical (root, node) distributions of one
                               launch are evaluated once and shared by the walks that need them */
    /* timing counters cover the PROFILED walk calls only (gg_set_profiling; by default every call) */
    double score_kernel_ms; /* cumulative HIP-event time of level_score_kernel (the dominant kernel) */
    int64_t score_launches;
    int64_t score_chunks;   /* 16-candidate work items those launches processed */
    int64_t score_rows;     /* neighbour rows those launches streamed */
    double bfs_kernel_ms;   /* cumulative HIP-event time of the BFS-tree kernel (gg_build_trees_device) */
    int64_t bfs_trees;      /* ... and the trees it built */
    int64_t score_dists;    /* (root, node) distributions the timed score launches evaluated (one current row each) */
    /* per-kernel HIP-event times of the PROFILED prepare / pass calls (same cadence as the walks), with the units they
     * processed: K2 pair_reward; K3 / K4 gradient kernel and K5 optimizer kernel of the discriminator / generator pass */
    double reward_kernel_ms;
    int64_t reward_pairs_timed;
    double d_grad_ms, d_opt_ms;
    int64_t d_pairs_timed, d_rows_timed;   /* pairs of those passes; table rows their optimizer kernels updated */
    double g_grad_ms, g_opt_ms;
    int64_t g_pairs_timed, g_rows_timed;
    int64_t d_passes_timed, g_passes_timed;
    int64_t g_walk_nodes_timed;            /* path nodes (= hops) of the gg_prepare_g calls counted in reward_pairs_timed */
    /* edge-score cache of the walk sampler: the score of a graph edge does not depend on the root, so a node's adjacency is
     * scored once per generator state and the (root, node) distributions of all roots gather from it */
    int64_t es_gathers;     /* (root, node) distributions that took their scores from the cache (no rows streamed) */
    int64_t es_nodes;       /* nodes whose whole adjacency was scored into the cache */
    int64_t score_gathers;  /* ... of the timed launches (the cadence of score_rows / score_dists) */
    int64_t score_nodes;
    int64_t walk_reruns;    /* sync-free walk launches that overflowed their learned buffer capacity / level count and were
                               repeated in sized mode (expected: the first launches of a workload, then none) */
} gg_counters;

typedef struct gg_ctx gg_ctx;

int gg_abi_version(void);
const char *gg_last_error(const gg_ctx *ctx);

/* ---- life cycle.  Replaces build_generator/build_discriminator + tf.Session init
 * (graph_gan.py:48-61, generator.py:11-15, discriminator.py:11-15): two [n_node, n_emb]
 * fp32 tables from the caller's init matrices, zero bias vectors, zero Adam slots. */
int gg_create(int32_t n_node, int32_t n_emb, const float *emb_gen, const float *emb_dis,
              const gg_config *cfg, gg_ctx **out);
int gg_destroy(gg_ctx *ctx);

/* ---- graph + BFS trees.
 * gg_set_graph_csr: the adjacency dict of utils.read_edges (utils.py:12-47) as CSR,
 * neighbour order = list order (it decides BFS child order and D-step positives). */
int gg_set_graph_csr(gg_ctx *ctx, const int64_t *rowptr /*[n_node+1]*/, const int32_t *col);

/* Trees cross the ABI in the REFERENCE'S SHAPE (graph_gan.py:90,96): for root slot r, node v's list
 * [father, child_0, ...] (root: [root, child...]) is nbr[nbr_base[r] + off[r*(n_node+1)+v] .. off[r*(n_node+1)+v+1]),
 * lists in node-id order; 2 * |component| - 1 entries per root.  Inside the context they live in BFS-order form
 * (pop order + first-child rank per rank, 8 bytes per node and root).
 * gg_host_build_trees: construct_trees (graph_gan.py:84-108) on host threads, no GPU, no ctx.
 * nbr == NULL sizes only.  Returns total entries (>= 0) or GG_E*. */
int64_t gg_host_build_trees(int32_t n_node, const int64_t *rowptr, const int32_t *col,
                            const int32_t *roots, int32_t n_roots,
                            int32_t *off /*[n_roots*(n_node+1)]*/, int32_t *nbr, int64_t *nbr_base /*[n_roots+1]*/,
                            int64_t cap, int32_t n_threads, int32_t *max_depth_out);

/* gg_build_trees: same, built in batches and uploaded into the context (replaces the pickle
 * cache load/construct branch, graph_gan.py:31-46).  Root slot i holds the tree of roots[i]. */
int gg_build_trees(gg_ctx *ctx, const int32_t *roots, int32_t n_roots, int32_t n_threads);
/* gg_build_trees_device: the same trees built ON THE GPU: one workgroup per root replays the reference's edge
 * stream (pop order x adjacency order) 4 096 edges at a time against a visited bitmap in LDS; a node is appended
 * at the first edge of the stream that reaches it.  Written straight into the resident BFS-order arrays. */
int gg_build_trees_device(gg_ctx *ctx, const int32_t *roots, int32_t n_roots);
/* gg_set_trees / gg_get_trees: upload / download trees in the reference's shape (tests, foreign caches; the
 * download shows the in-place D-mode mutations, graph_gan.py:258-259, as father entries of -1). */
/* LAZY trees (ABI 7).  The walks of one prepare call read a few hundred of a tree's children lists (graph_gan.py:249-250: the
 * list of the node the walk stands on) -- 5e-5 of what construct_trees (:84-108) writes per root on the 10^6-node bench graph --
 * and the tree of a root that cannot stay resident is built, walked twice and dropped.  In lazy mode gg_build_trees_device builds
 * a root's tree exactly only THROUGH the last level whose expansion is known to fit a node limit (nodes so far + adjacency entries
 * of the level <= limit); the children list of a deeper node is resolved by the first walk that stands on it, from the visited
 * set of the exact levels and their BFS ranks (a child of v = a neighbour outside the set whose first queue neighbour is v, in
 * adjacency order: the list the BFS would have appended, entry for entry) up to two levels below the exact ones.  A root whose
 * walks go deeper -- or whose pool of resolved lists is full -- gets its whole tree behind the scenes and the launch is repeated:
 * every gg_walk_sample / gg_prepare_* result is the whole trees' result, bit for bit (tested against the oracle's).
 * mode: 0 = whole trees (gg_get_trees / gg_save_trees / gg_get_tree_order need them), 1 = lazy, -1 (default) = lazy for graphs of
 * 2^18 nodes and more (GG_LZ_AUTO_NODES); GG_TREE_LAZY overrides.  node_cap: the limit per root; 0 = the default rule: 3/8 of the nodes
 * (at least 65 536; GG_LZ_CAP), except that the root's first two levels may expand up to the node count (GG_LZ_EASY levels), and a
 * root whose component holds <= 65 536 nodes gets its whole tree; node_cap > 0 = exactly that limit for every level and as the
 * whole-tree bound (tests).  gg_tree_info reports, for lazy trees, a depth no walk exceeds.
 * gg_lazy_stats: out24 = {resident trees are lazy, smallest exact level of the lazy slots, slots rebuilt whole so far, launches
 * repeated for it, exact nodes the BFS wrote, pool entries reserved by resolutions, lazy slots, deepest exact level; of the
 * resident build: lists resolved at depth 0 / 1 / 2, candidates judged, 16-entry scan rounds, most rounds of one list, longest
 * adjacency resolved, lists resolved by a whole workgroup (long adjacencies); lazy slots whose exact level is 0 .. 7}.
 * gg_get_lazy_trees (tests): the raw arrays -- info4[slot] = {first rank without a built list, exact ranks, their level,
 * capacity of the segment}, base[slot], then order / cstart / edge / pair over *n_entries entries (cstart: + n_roots). */
int gg_set_tree_mode(gg_ctx *ctx, int32_t mode, int64_t node_cap);
/* gg_debug_words (diagnostics): n of the context's 2 048 device counter words from `first` on. */
int gg_debug_words(gg_ctx *ctx, int32_t first, int32_t n, uint64_t *out);
int gg_lazy_stats(gg_ctx *ctx, int64_t *out24);
int gg_get_lazy_trees(gg_ctx *ctx, int64_t *n_entries, int32_t *info4, int64_t *base, int32_t *order, int32_t *cstart, int32_t *edge, uint64_t *pair);
int gg_set_trees(gg_ctx *ctx, const int32_t *roots, int32_t n_roots, const int32_t *off,
                 const int32_t *nbr, const int64_t *nbr_base, int32_t max_depth);
int gg_tree_info(const gg_ctx *ctx, int32_t *n_roots, int64_t *n_entries, int32_t *max_depth);
int gg_tree_roots(const gg_ctx *ctx, int32_t *roots /*[n_roots]*/);  /* root node of every resident slot */
/* gg_save_trees / gg_load_trees: the tree cache, replacing the pickle of graph_gan.py:31-46 (config.cache_filename).
 * One flat file holding the resident BFS-order arrays as built (roots, bases, pop order, first-child ranks; the
 * reference also pickles before any in-place mutation, :45) behind a header with the graph's fingerprint: a cache
 * built from another graph is refused with GG_EINVAL, a truncated or foreign file with GG_EIO (nothing loaded). */
int gg_save_trees(gg_ctx *ctx, const char *path);
int gg_load_trees(gg_ctx *ctx, const char *path);
int gg_get_trees(gg_ctx *ctx, int32_t *off, int32_t *nbr, int64_t *nbr_base);
/* gg_get_tree_order: the resident trees in their internal BFS-ORDER form, slot by slot: base[r] =
 * first entry of slot r (n_roots + 1 values); order[base[r] + i] = node of BFS pop rank i (the reference's queue,
 * graph_gan.py:96-107); cstart[base[r] + r + i] = rank of the first child of rank i (C_r + 1 values per slot); edge[base[r] + i]
 * = CSR index of the graph edge (father -> node) the BFS appended rank i at (-1 for the root) -- what the walk sampler's
 * edge-score cache is indexed by.  *edges_valid = 0 when the resident trees carry no edge indices (uploaded lists that are
 * no subgraph of the resident graph).  Any pointer may be NULL. */
int gg_get_tree_order(gg_ctx *ctx, int64_t *base, int32_t *order, int32_t *cstart, int32_t *edge, int32_t *edges_valid);

/* ---- K1 walk_sample.  Replaces GraphGAN.sample (graph_gan.py:225-270) including the
 * all_score fetch (:238, generator.py:21), utils.softmax (utils.py:131-133) and
 * np.random.choice (:262).  For each i: n_walks[i] walks on the tree in slot slots[i]
 * (D-mode: for_d = 1, n_walks = len(graph[root]), :190-191; G-mode: n_sample_gen, :210).
 * Walk w = walk_ptr[i] + j writes samples[w] (end node, -1 if the root aborted),
 * paths[w*stride ..] = [root, ..., end, prev-of-end], path_len[w] (0 if aborted).
 * Host output pointers may be NULL (results stay resident for gg_prepare_*).
 * Uniforms: Philox4x32-10(key = seed; counter = hop, j, root id, stream) -> results do not
 * depend on slot order, batching or GPU count.  Arithmetic: DESIGN.md section 3. */
int gg_walk_sample(gg_ctx *ctx, const int32_t *slots, const int32_t *n_walks, int32_t n_slots,
                   int32_t for_d, uint64_t seed, uint32_t stream,
                   int32_t *samples, int32_t *paths, int32_t *path_len, int32_t stride,
                   int32_t *root_status);

/* gg_walk_info / gg_get_walks: shape and contents of the walk outputs left resident by the last gg_walk_sample /
 * gg_prepare_d / gg_prepare_g call (what GraphGAN.sample returned for those roots, graph_gan.py:191,210): total walks,
 * path stride and slot count; then samples [total], paths [total * stride], path_len [total], root_status [n_slots]
 * (any pointer may be NULL).  Used by parity tests that check the walks INSIDE a prepare call. */
int gg_walk_info(const gg_ctx *ctx, int64_t *total_walks, int32_t *stride, int32_t *n_slots);
int gg_get_walks(gg_ctx *ctx, int32_t *samples, int32_t *paths, int32_t *path_len, int32_t *root_status);

/* ---- prepared sample buffers (device resident).
 * gg_prepare_d: prepare_data_for_d (graph_gan.py:182-202) for the given root slots: D-mode
 * walks (n_walks = CSR degree), then rows [pos..., neg...] per non-aborted root, in slot order.
 * gg_prepare_g: prepare_data_for_g (:204-223): n_sample walks per root, window pairs
 * (get_node_pairs_from_path, :272-291) and reward (discriminator.py:33-34) for all pairs.  Its walks read only the
 * generator's tables and the trees, so they are enqueued on a side stream and run beside a gg_d_pass that is still
 * in flight (gg_set_profiling); pairs and rewards follow on the main stream, behind that discriminator update. */
int gg_prepare_d(gg_ctx *ctx, const int32_t *slots, int32_t n_slots, uint64_t seed, uint32_t stream,
                 int64_t *n_rows_out, int32_t *root_status /*[n_slots] or NULL*/);
int gg_get_d_data(gg_ctx *ctx, int32_t *center, int32_t *neighbor, float *label);
int gg_prepare_g(gg_ctx *ctx, const int32_t *slots, int32_t n_slots, int32_t n_sample, uint64_t seed,
                 uint32_t stream, int64_t *n_pairs_out, int32_t *root_status);
/* Optional head start for the gg_prepare_g that follows a discriminator update: enqueue its walks NOW -- on the side stream,
 * without any host synchronisation -- typically between gg_prepare_d and gg_d_pass, so that they run beside the whole
 * discriminator pass instead of starting once the host has enqueued it (graph_gan.py:204-216 samples from the generator
 * only; the rewards of :220-222, which need the updated discriminator, stay in gg_prepare_g).  The next gg_prepare_g with
 * the SAME (slots, n_sample, seed, stream) adopts the launch and returns exactly what it would have returned without
 * this call.  Any other call that needs the walk buffers, the trees or the generator's tables -- another walk launch,
 * gg_get_walks, gg_get_g_data, gg_g_step / gg_g_pass, gg_set_embeddings / gg_set_bias(0), gg_load_state, a tree or graph
 * call -- first waits for the begun launch and drops it; a later gg_prepare_g then launches anew.  Allowed in between
 * without losing the head start: gg_d_step / gg_d_pass, gg_get_d_data, the getters and gg_synchronize. */
int gg_prepare_g_begin(gg_ctx *ctx, const int32_t *slots, int32_t n_slots, int32_t n_sample, uint64_t seed, uint32_t stream);
/* The (node_1, node_2) arrays of gg_prepare_g are expanded from its walks on first use -- gg_get_g_data, or a gg_g_pass in
 * minibatches -- which must therefore come before the next walk launch of the context (gg_prepare_d / gg_prepare_g /
 * gg_walk_sample); later it is GG_EINVAL.  Rewards, and whole-batch passes over the walks, do not need them. */
int gg_get_g_data(gg_ctx *ctx, int32_t *node_1, int32_t *node_2, float *reward);

/* ---- an epoch over ROOT BATCHES (ABI 5).  The reference keeps the tree of every root resident (self.trees, graph_gan.py:31-46)
 * and prepare_data_for_d / prepare_data_for_g visit every root (:188, :208) before the passes run over all rows (:149-157,
 * :168-176).  N trees are N^2 entries (12 TB at 10^6 nodes): where they cannot all be resident, the same schedule runs with
 * one batch of trees in HBM at a time:
 *   gg_epoch_begin   empty the accumulated discriminator rows (reset_d) and / or generator pairs (reset_g);
 *   gg_epoch_add     for the given ROOTS (node ids, not slots): their BFS trees are built on the GPU into slots 0 .. n_roots-1
 *                    (whatever was resident is replaced), the roots' Q3 bits -- father entries that D-mode walks of EARLIER
 *                    epochs removed for good, graph_gan.py:258-259 -- are restored from a store that outlives the trees; do_d:
 *                    gg_prepare_d on them (seed, stream_d), bits saved back, rows appended; do_g: gg_prepare_g (n_sample, seed,
 *                    stream_g), window pairs appended.  do_d and do_g in one call share the trees: the G-mode walks read only
 *                    the generator, the trees and the Q3 bits the D-mode walks of the same root have just set -- nothing the
 *                    discriminator's passes change -- so one BFS per root serves both phases of an outer epoch.  Batches are
 *                    appended in call order; *rows_total_out / *pairs_total_out = accumulated so far.  gg_get_walks /
 *                    gg_get_trees afterwards show the batch's last launch / its trees (mutations included).
 *   gg_epoch_commit  which = 1: the accumulated rows become the resident prepared data of gg_d_pass / gg_get_d_data;
 *                    which = 0: the rewards of ALL accumulated pairs are evaluated now (graph_gan.py:220-222, with the
 *                    discriminator as its passes left it) and the pairs become the data of gg_g_pass / gg_get_g_data.
 *                    With replicas this is where the ranks exchange their counts (once per epoch, not per batch).
 * Rows / pairs equal those of the all-resident calls over the same roots in the same order (tested bit for bit).
 * gg_q3_clear forgets all mutations (a fresh process of the reference: its pickle is written before any, :45);
 * gg_q3_get reads the store: word_off[v] .. word_off[v + 1] = the ceil(deg(v) / 32) words of root v, bit j = the father entry of
 * its (j + 1)-th tree child was removed.  The store is also what gg_epoch_add leaves in the resident slots' own Q3 rows. */
int gg_epoch_begin(gg_ctx *ctx, int32_t reset_d, int32_t reset_g);
int gg_epoch_add(gg_ctx *ctx, const int32_t *roots, int32_t n_roots, int32_t do_d, int32_t do_g, int32_t n_sample, uint64_t seed,
                 uint32_t stream_d, uint32_t stream_g, int64_t *rows_total_out, int64_t *pairs_total_out);
int gg_epoch_commit(gg_ctx *ctx, int32_t which, int64_t *n_out);
int gg_q3_clear(gg_ctx *ctx);
int gg_q3_get(gg_ctx *ctx, int64_t *word_off /*[n_node + 1] or NULL*/, uint32_t *words /*[word_off[n_node]] or NULL*/);

/* gg_d_pass / gg_g_pass: one inner epoch over the prepared rows = the minibatch loops
 * graph_gan.py:149-157 / :168-176: for each s in starts (the caller's shuffled start_list),
 * one optimizer step on rows [s, min(s+batch, n)). */
int gg_d_pass(gg_ctx *ctx, const int64_t *starts, int64_t n_batches, int32_t batch_size);
int gg_g_pass(gg_ctx *ctx, const int64_t *starts, int64_t n_batches, int32_t batch_size);

/* ---- the sess.run call sites with host buffers.
 * gg_pair_reward: sess.run(discriminator.reward) (graph_gan.py:220-222, discriminator.py:21-24,33-34)
 * gg_d_step:      sess.run(discriminator.d_updates) (graph_gan.py:154-157, discriminator.py:26-32)
 * gg_g_step:      sess.run(generator.g_updates)     (graph_gan.py:173-176, generator.py:22-31) */
int gg_pair_reward(gg_ctx *ctx, const int32_t *u, const int32_t *v, int64_t n, float *out);
int gg_d_step(gg_ctx *ctx, const int32_t *u, const int32_t *v, const float *label, int32_t n);
int gg_g_step(gg_ctx *ctx, const int32_t *u, const int32_t *v, const float *reward, int32_t n);

/* gg_all_score: sess.run(generator.all_score) (graph_gan.py:238, generator.py:21) for the given rows:
 * out[i * n_node + j] = g_rows[i] . g_j + b_g[j]; rows == NULL -> every row (n_rows ignored, out is
 * [n_node, n_node]).  Exact fp32 on the matrix cores (v_mfma_f32_32x32x2_f32, k-ordered fmaf chain).
 * The engine itself never needs it (gg_walk_sample scores tree neighbours on demand); it is here for
 * callers that still want score rows. */
int gg_all_score(gg_ctx *ctx, const int32_t *rows, int32_t n_rows, float *out);

/* gg_all_score_reduce: the same score rows STREAMED through a fused consumer instead of being materialised: for each
 * requested row i (rows == NULL: every node) the maximum of S[i, :], its column (first maximum, like numpy argmax) and
 * log sum_j exp(S[i, j]) -- the normaliser of the full softmax over all nodes (row_lse may be NULL with want_lse = 0).
 * Nothing of size n_rows x n_node exists at any time.  precision 0: exact fp32 scores on v_mfma_f32_32x32x2_f32;
 * precision 1: a bf16 copy of the table (round to nearest even) on v_mfma_f32_32x32x16_bf16, fp32 accumulate.
 * kernel_ms_out (may be NULL): HIP-event time of the tile stream.  Replaces what a caller of generator.all_score
 * (generator.py:21) would do with the N x N matrix at sizes where it cannot exist (BASELINE.json configs[4]). */
int gg_all_score_reduce(gg_ctx *ctx, const int32_t *rows, int32_t n_rows, int32_t precision, int32_t want_lse, float *row_max,
                        int32_t *row_argmax, float *row_lse, double *kernel_ms_out);

/* gg_topk_scores: streamed top-K retrieval (recommendation).  For each requested node u (rows == NULL: every node, n_rows
 * ignored; repeated rows allowed) and the table E of model `which` (0 = generator, 1 = discriminator):
 *   score       s(u, v) = E[u] . E[v], fp32, NO bias (the evaluator's score, link_prediction.py:26-27);
 *   eligible    exclude = 0: every node; exclude = 1: every node but u itself and u's neighbours in the resident training
 *               graph (gg_set_graph_csr; duplicates in a list are fine; without a graph: GG_EINVAL);
 *   result      the first k eligible columns in the order (score descending, column ascending):
 *               out_col[n_rows][k] (int32) and out_score[n_rows][k] (fp32), row-major; a row with fewer than k eligible
 *               columns is padded with -1 / -inf.  1 <= k <= 256.
 * precision 0: exact fp32 (v_mfma_f32_32x32x2_f32, the k-ordered fmaf chain of gg_all_score): indices and scores are those of
 * a stable sort of the fp32 score rows.  precision 1: a bf16 copy of the table (round to nearest even) on
 * v_mfma_f32_32x32x16_bf16, fp32 accumulate (n_emb <= 512).  Nothing of size n_rows x n_node exists at any time: rows are
 * processed in internal passes of 4 096 with bounded device scratch.  kernel_ms_out (may be NULL): HIP-event time of the tile
 * streams and the device merges, summed over the passes (the bf16 copy excluded, as in gg_all_score_reduce). */
int gg_topk_scores(gg_ctx *ctx, int32_t which, const int32_t *rows, int32_t n_rows, int32_t k, int32_t precision, int32_t exclude,
                   int32_t *out_col, float *out_score, double *kernel_ms_out);

/* gg_rank_scores (additive: a new symbol, the ABI number stays): full-ranking link evaluation.  For each query i the exact
 * position of the target v[i] among ALL candidate columns of row u[i] of S = E E^T, table E of model `which` (0 = generator,
 * 1 = discriminator):
 *   score       s(u, c) = E[u] . E[c], fp32, NO bias -- the bits the tile stream of that precision produces for row u, column c:
 *               precision 0: v_mfma_f32_32x32x2_f32, the k-ordered fmaf chain from 0.0, bit-identical to gg_all_score with zero
 *               bias (whose added +0.0 turns a chain that ends at -0.0 into +0.0: the one difference, and a tie); precision 1: a bf16 copy of the table (round to nearest even) on v_mfma_f32_32x32x16_bf16, fp32
 *               accumulate (n_emb <= 512);
 *   order       gg_topk_scores' order: score descending, column ascending, -0 counting as +0 (the key ord(score) << 32 | ~col
 *               of topk_score.hip); "c is ahead of v" below means c comes before v in it;
 *   candidates  exclude = 0: every node; exclude = 1: every node but u[i] itself and u[i]'s neighbours in the resident training
 *               graph (gg_set_graph_csr; duplicates in a list are fine; without a graph: GG_EINVAL).  The target v[i] is ALWAYS a
 *               candidate, also where that rule would drop it: u[i] == v[i] and a target that is a training neighbour are legal;
 *   results     rank_out[i]   = 1 + the number of candidates c != v[i] ahead of v[i]              (int32 [m]);
 *               n_cand_out[i] = the number of candidates, the target included once               (int32 [m], or NULL);
 *               score_out[i]  = s(u[i], v[i])                                                     (fp32 [m], or NULL).
 *               With `exclude` equal on both sides and an eligible target: rank <= k if and only if gg_topk_scores returns v[i]
 *               at position rank - 1 of row u[i], with the same score bits.
 * 1 <= m <= 2^31 - 1; an id outside [0, n_node) is GG_EINVAL (the text names gg_rank_scores and the first bad index; nothing is
 * launched).  Repeated queries are allowed and give identical outputs; a query's outputs depend on nothing but its own (u, v) --
 * not on the other queries, their order or the internal passes -- and, the counts being integers, are identical from run to
 * run.  Non-finite scores: unspecified.  Nothing of size m x n_node exists at any time: the queries are processed in internal
 * passes of 4 096 with bounded device scratch.  kernel_ms_out (may be NULL): HIP-event time of the tile streams plus the
 * threshold / correction kernels, summed over the passes (the bf16 copy excluded, as in gg_topk_scores). */
int gg_rank_scores(gg_ctx *ctx, int32_t which, const int32_t *u, const int32_t *v, int64_t m, int32_t precision, int32_t exclude,
                   int32_t *rank_out, int32_t *n_cand_out, float *score_out, double *kernel_ms_out);

/* gg_graph_softmax (ABI 9): the generator's distribution G(v | root) of the tree in each given slot, exactly -- the law of the
 * end node of ONE walk of gg_walk_sample on the same slot, mode and tables.  The reference defines it only by how
 * GraphGAN.sample walks (graph_gan.py:225-270; scores all_score = E_g E_g^T + b_g, generator.py:21).  With the reference's
 * lists tree[v] = [father, children...] of the slot's root rho, the candidates N(v) of a reached node v are: at the root its
 * children (tree[root][1:], :249); elsewhere father + children, the father dropped where the slot's Q3 bit of v is set (a D-mode
 * walk removed it for good, :258-259) or, with GG_GS_FOR_D, where the father is rho (:256-259).  With
 *   q(w | v) = exp(s(v, w)) / sum_{x in N(v)} exp(s(v, x)),  s(v, w) = g_v . g_w + b_g[w]      (the mathematical softmax:
 *   no S2 cut at -28, no S3 truncation -- they differ from it by less than 1e-12)
 *   reach(rho) = 1, reach(c) = reach(v) q(c | v) for every child c of v;
 *   P(v) = reach(v) q(father(v) | v) if the father is in N(v), else 0 (P(rho) = 0);
 *   A = sum of reach(v) over reached v with N(v) empty (the walk aborts, ``return None, None``): a root without children, a
 *       G-mode depth-1 leaf whose father entry Q3 removed, a D-mode depth-1 leaf (``node_neighbor == [root]``);
 * sum_v P(v) + A = 1.  Outputs are LOG-probabilities in fp32 (P = 0 -> -inf: the root, unreached nodes, dropped fathers):
 *   logp       [n_slots * n_node] dense rows by node id, or NULL;
 *   q_off / q_node / q_logp   queried pairs instead (or as well): q_logp[j] = log P of node q_node[j] in slot k for
 *              q_off[k] <= j < q_off[k + 1] (q_off[0] = 0; q_off and q_logp both NULL or both given);
 *   abort_mass [n_slots] A, or NULL.
 * flags: GG_GS_FOR_D -- the D-mode walk rules; GG_GS_Q3_STORE -- Q3 bits from the persistent store of gg_epoch_* (by root node;
 * no store yet = no bits) instead of the slots' own rows.
 * Arithmetic: edge scores in float64 from the fp32 tables (a private buffer filled once per generator state -- the walks' own
 * edge-score cache is not touched, so walks before and after the call are identical); max, log-sum-exp and log reach in
 * float64, every sum in a fixed order: a slot's results do not depend on the other slots of the call, their order or the
 * internal passes of up to 4 096 slots (bounded device scratch), and repeated calls give identical bits.
 * kernel_ms_out (may be NULL): HIP-event time of the sweeps summed over the passes (the edge-score fill excluded).
 * GG_EINVAL: lazy resident trees (build them whole: gg_set_tree_mode(ctx, 0) with node_cap 0), trees without edge indices
 * (gg_get_tree_order's edges_valid == 0), a slot or q_node out of range, a non-finite generator table.  A gg_prepare_g_begin
 * launch is waited for and dropped (the call reads the trees and the generator). */
#define GG_GS_FOR_D     1  /* D-mode walk rules */
#define GG_GS_Q3_STORE  2  /* Q3 bits from the persistent store of gg_epoch_* (no store yet = no bits) instead of the slots' own */
int gg_graph_softmax(gg_ctx *ctx, const int32_t *slots, int32_t n_slots, int32_t flags,
                     float *logp /*[n_slots * n_node] or NULL*/,
                     const int64_t *q_off /*[n_slots + 1] or NULL*/, const int32_t *q_node, float *q_logp,
                     float *abort_mass /*[n_slots] or NULL*/, double *kernel_ms_out);

/* ---- skip-gram pre-training rows (additive entry points; GG_ABI_VERSION stays 9: no existing symbol, struct or behaviour
 * changes).  The reference starts from the pre_train .emb files of an external DeepWalk / node2vec run (config.py:33-34,
 * utils.read_embeddings); these two calls produce, on the device, the rows that train such a table with the machinery that is
 * already here: gg_d_pass on (center, neighbor, label) rows with sigmoid cross-entropy IS one-table skip-gram with negative
 * sampling.  SAMPLING CONTRACT -- exact integer arithmetic throughout, so any decomposition over threads, calls or GPUs gives
 * the same rows (the stance of S3-S5):
 *   P1 uniform draw   m = uniform53(seed, stream, root = start node id, walk = w, hop): Philox4x32-10, counter (hop, w, start, stream),
 *                     key seed (S4); t(K) = threshold(m, K) = floor(m * K / 2^53) (S5).
 *   P2 walk           start node s, walk w in [0, walks_per_start): path[0] = s; for h = 1 .. walk_len - 1 with cur = path[h - 1],
 *                     k = deg(cur): k == 0 ends the walk (path_len = h), else path[h] = col[rowptr[cur] + t(k)] drawn with hop = h.
 *                     Walks are stored in the order (start index, w); entries behind path_len are -1.
 *   P2b biased walk   (node2vec; replaces P2 while gg_pretrain_set_walk_bias holds unequal weights).  Walk bias: three integers
 *                     (w_ret, w_com, w_out), each in [1, 65536], M = the largest.  CLASS of a candidate x at hop h, with
 *                     prev = path[h - 2], tested in this order: x == prev -> w_ret; x occurs in adj(prev), the resident list of
 *                     prev exactly as handed to gg_set_graph_csr (duplicates are fine, a directed CSR stays well defined) -> w_com;
 *                     otherwise -> w_out.  Hop h with cur = path[h - 1], k = deg(cur), e0 = rowptr[cur]: k == 0 ends the walk
 *                     as in P2.  If h == 1, or k == 1, or w_ret == w_com == w_out: exactly P2 (one draw with hop word h,
 *                     path[h] = col[e0 + t(k)]).  Otherwise trials r = 0 .. R - 1, R = 32: the candidate
 *                     x_r = col[e0 + threshold(m_c(r), k)] is drawn from the list in FILE order, m_c(0) = uniform53(seed, stream,
 *                     start, w, hop = h) and m_c(r >= 1) uses hop word 2^31 + 256 r + h; it is accepted iff class(x_r) == M or
 *                     threshold(m_a(r), M) < class(x_r), where m_a(r) uses hop word 2^30 + 256 r + h; the first accepted
 *                     candidate is path[h].  If all R trials are rejected, one exact draw: W = sum of class(col[e]) over the list
 *                     of cur in file order, t = threshold(m_f, W) with hop word 2^31 + 256 R + h for m_f, and path[h] is the first
 *                     list entry whose inclusive prefix sum of class weights exceeds t.
 *                     The hop words are disjoint from every P2 / P4 draw: h <= 255 and the negatives' hop words stay below 2^30
 *                     (walk_len + pairs * n_neg <= 256 + 8192 * 64).  Consequences: every step has exactly the node2vec law
 *                     class(x) / W per list entry (rejection and the exact draw both realise it); equal weights reproduce P2 BIT
 *                     FOR BIT; draws are keyed by (start, w, hop word) only, so any decomposition gives the same paths.
 *   P3 pairs          over the WHOLE path of length l (there is no back-step entry to drop, unlike get_node_pairs_from_path,
 *                     graph_gan.py:272-291): for i ascending and j in [max(i - window, 0), min(i + window, l - 1)] ascending, j != i,
 *                     pair number p is (path[i], path[j]).
 *   P4 negatives      pair p, q in [0, n_neg): drawn with hop = walk_len + p * n_neg + q.  Noise distribution from the uint32
 *                     weights of gg_pretrain_set_noise: C_j = inclusive prefix sums (uint64), W = C_{N-1} >= 1, node = the first j
 *                     with C_j > t(W); without weights uniform: node = t(N).  While the node equals the pair's centre or its
 *                     context: node = (node + 1) mod N (at most two steps; n_node >= 3 required).
 *   P5 rows           walks in order, pairs in order; each pair gives (centre, context, 1.0) and then its n_neg rows
 *                     (centre, neg_q, 0.0).  A walk of length l gives (1 + n_neg) * sum_i [min(i, window) + min(l - 1 - i, window)]
 *                     rows, so row offsets are a scan over path_len.
 *   limits            1 <= walk_len <= 256, 1 <= window <= 16, 0 <= n_neg <= 64, walks_per_start >= 1; repeated start nodes are
 *                     allowed and give identical walks.
 * gg_pretrain_set_noise: weight[n_node] (copied; all zero: GG_EINVAL) or NULL = uniform.  gg_set_graph_csr drops the table.
 * gg_pretrain_set_walk_bias: the walk bias of P2b, held in the context (default (1, 1, 1)) and KEPT across gg_set_graph_csr -- it
 * does not depend on the graph, unlike the noise table.  A weight of 0 or above 65536: GG_EINVAL (no graph needed).  With equal
 * weights gg_prepare_pretrain launches the uniform walk kernel exactly as before; with unequal weights the biased kernel, which
 * tests membership by binary search in a per-node SORTED copy of the lists (built on first use after gg_set_graph_csr, shared
 * with gg_topk_scores' exclusion; candidates are still drawn from the file-order lists), then the same count / scan / fill.
 * gg_prepare_pretrain: needs gg_set_graph_csr.  REPLACES the resident discriminator rows exactly as a gg_prepare_d call does
 * (gg_get_d_data and gg_d_pass then work on them unchanged); *n_rows_out = their number; paths [n_starts * walks_per_start *
 * walk_len] and path_len [n_starts * walks_per_start] may be NULL.  It has path buffers of its own and neither reads nor writes
 * the walk sampler's buffers, the trees, the edge-score / distribution caches or the generator: walks and graph-softmax results
 * around it are unchanged and a gg_prepare_g_begin launch stays valid.  One host synchronisation (the row total); when even the
 * bound (every walk at full length) exceeds 2^31 - 1 rows, a second one decides on the exact total.
 * GG_EINVAL: no graph, a limit violated, a start out of range, an attached communicator (single rank only), a call between
 * gg_epoch_begin(reset_d) / gg_epoch_add(do_d) and the matching gg_epoch_commit(1).  GG_ECAPACITY: more than 2^31 - 1 rows (or
 * walks) in one call.  With profiling cadence 1 (gg_set_profiling) gg_counters.last_kernel_ms = HIP-event time of the row (fill)
 * kernel and walk_kernel_ms / walk_launches also count this call's walk kernel (the uniform or the biased one). */
int gg_pretrain_set_noise(gg_ctx *ctx, const uint32_t *weight /*[n_node] or NULL = uniform*/);
int gg_pretrain_set_walk_bias(gg_ctx *ctx, uint32_t w_ret, uint32_t w_com, uint32_t w_out /*each in [1, 65536]*/);
int gg_prepare_pretrain(gg_ctx *ctx, const int32_t *starts, int32_t n_starts, int32_t walks_per_start, int32_t walk_len,
                        int32_t window, int32_t n_neg, uint64_t seed, uint32_t stream, int64_t *n_rows_out,
                        int32_t *paths /*[n_starts*walks_per_start*walk_len] or NULL*/, int32_t *path_len /*or NULL*/);

/* ---- node classification (additive entry points; GG_ABI_VERSION stays 9: no existing symbol, struct or behaviour changes).
 * The GraphGAN paper's third application: multinomial logistic regression on the FROZEN rows of table `which` (0 = generator,
 * 1 = discriminator), gathered by node id from the resident table -- nothing of size m x n_emb crosses to the host.  With
 * C = n_class, d = n_emb, W fp32 [C, d] row-major, b fp32 [C], rows i = 0 .. m - 1 (nodes[i], labels[i]):
 *   z_i  = W . E[nodes[i]] + b,   p_i = softmax(z_i) (max-subtracted)
 *   loss = -(1/m) sum_i log p_i[labels[i]] + (l2 / 2) |W|^2                  (the bias is not regularised)
 *   gW   = (1/m) sum_i (p_i - onehot(labels[i])) E[nodes[i]]^T + l2 W,   gb = (1/m) sum_i (p_i - onehot(labels[i]))
 * gg_classifier_lossgrad: loss_out[1], gW_out[C * d], gb_out[C] at the given (W, b): ONE fused sweep (every row is read once;
 *   both products on v_mfma_f32_32x32x2_f32, fp32 throughout) and a reduction.
 * gg_classifier_fit: `iters` steps of full-batch Adam (beta1 = 0.9, beta2 = 0.999, eps = 1e-8, bias-corrected, step count from
 *   1: m_t = b1 m + (1 - b1) g, v_t = b2 v + (1 - b2) g^2, theta -= lr (m_t / (1 - b1^t)) / (sqrt(v_t / (1 - b2^t)) + eps)) on
 *   (W, b) from the values in W_inout / b_inout, which receive the result.  loss_out[t] (may be NULL) is the loss at the
 *   parameters BEFORE update t.  All iterations are enqueued on the engine's stream behind one another; one synchronisation
 *   at the end.  ms_out (may be NULL): HIP-event time of the iterations.
 * gg_classifier_predict: pred_out[i] = argmax_c z_i[c], ties to the LOWEST class; logits_out (may be NULL) [m, C] row-major.
 * limits       2 <= n_class <= 128, n_emb <= 256, 1 <= m <= 2^31 - 1, labels in [0, n_class), node ids in [0, n_node) and
 *              free to repeat; a class without a row is legal; iters >= 1, lr > 0, l2 >= 0.  Anything else: GG_EINVAL, the
 *              gg_last_error text names the limit, nothing is launched.
 * determinism  the rows are split over a grid that depends on m alone (not on the device), every workgroup writes its
 *              partial sums to a stage, a second kernel adds the stage in a fixed order; there are no floating-point
 *              atomics: two calls with the same inputs and table give the same bits. */
int gg_classifier_lossgrad(gg_ctx *ctx, int which, const int32_t *nodes, const int32_t *labels, int64_t m, int n_class,
                           const float *W, const float *b, float l2, float *loss_out, float *gW_out, float *gb_out);
int gg_classifier_fit(gg_ctx *ctx, int which, const int32_t *nodes, const int32_t *labels, int64_t m, int n_class,
                      int iters, float lr, float l2, float *W_inout, float *b_inout, float *loss_out /* [iters] or NULL */, double *ms_out);
int gg_classifier_predict(gg_ctx *ctx, int which, const int32_t *nodes, int64_t m, int n_class, const float *W, const float *b,
                          int32_t *pred_out, float *logits_out /* NULL or [m, n_class] */);

/* ---- multi-label node classification (additive entry points; GG_ABI_VERSION stays 9).  The paper's labelled datasets
 * (BlogCatalog, Wikipedia) give a node several labels: one-vs-rest logistic regression, one binary problem per class, on the
 * same frozen rows, under the limits of gg_classifier_* above.  Labels are a multi-hot mask label_bits uint32 [m][CW],
 * CW = ceil(n_class / 32): bit c & 31 of word c >> 5 is set when row i has class c.  A row with no label, or with every label,
 * is legal; a bit at a position >= n_class is GG_EINVAL (the text names the row and the bit).
 *   z_i  = W . E[nodes[i]] + b,   y_ic = bit c of row i
 *   loss = (1/m) sum_i sum_c [softplus(z_ic) - y_ic z_ic] + (l2 / 2) |W|^2    (every class normalised by m; the bias is not regularised)
 *   gW   = (1/m) sum_i (sigmoid(z_i) - y_i) E[nodes[i]]^T + l2 W,   gb = (1/m) sum_i (sigmoid(z_i) - y_i)
 * in the stable forms, with e = exp(-|z|): softplus(z) = max(z, 0) + log1p(e), sigmoid(z) = z >= 0 ? 1 / (1 + e) : e / (1 + e).
 * A logit of +-200 gives a finite loss and a gradient entry of exactly 0 - y or 1 - y; the loss at zero parameters is
 * n_class log 2.
 * gg_classifier_ml_lossgrad / gg_classifier_ml_fit: as gg_classifier_lossgrad / gg_classifier_fit -- the same fused sweep (its
 *   per-row loss stage is the only difference), the same stage and reduction, the same Adam (constants, bias correction, step
 *   count; loss_out[t] = the loss BEFORE update t) and the same determinism: a grid that depends on m alone, partials added in a
 *   fixed order, no floating-point atomics, the same inputs give the same bits.
 * gg_classifier_ml_predict: pred_bits [m][CW] in the layout of label_bits; logits_out (may be NULL) [m, n_class].  The classes
 *   of a row are totally ordered by logit descending, then class ascending.  With k [m]: row i gets the first k[i] classes of
 *   that order (the customary protocol passes the row's true label count); 0 <= k[i] <= n_class, otherwise GG_EINVAL naming the
 *   row.  With k == NULL: the classes with z > 0, strictly (an exact 0 is not predicted).  Unspecified on non-finite logits. */
int gg_classifier_ml_lossgrad(gg_ctx *ctx, int which, const int32_t *nodes, const uint32_t *label_bits, int64_t m, int n_class,
                              const float *W, const float *b, float l2, float *loss_out, float *gW_out, float *gb_out);
int gg_classifier_ml_fit(gg_ctx *ctx, int which, const int32_t *nodes, const uint32_t *label_bits, int64_t m, int n_class,
                         int iters, float lr, float l2, float *W_inout, float *b_inout, float *loss_out /* [iters] or NULL */, double *ms_out);
int gg_classifier_ml_predict(gg_ctx *ctx, int which, const int32_t *nodes, int64_t m, int n_class, const float *W, const float *b,
                             const int32_t *k /* [m] or NULL */, uint32_t *pred_bits /* [m][CW] */, float *logits_out /* NULL or [m, n_class] */);

/* ---- learned link prediction (additive entry points; GG_ABI_VERSION stays 9).  The protocol of the GraphGAN and node2vec
 * papers: a binary operator on the two endpoint rows of an edge, logistic regression on the result.  The rows are the FROZEN
 * rows of table `which`, gathered by node id from the resident table; nothing of size m x n_emb crosses to the host.  With
 * d = n_emb, w fp32 [d], b fp32 [1], edges i = 0 .. m - 1 (u[i], v[i]) with labels y[i] in {0, 1}:
 *   x_i  = op(E[u[i]], E[v[i]]) elementwise:  op 0 Hadamard a b, 1 average (a + b) 0.5f, 2 L1 |a - b|, 3 L2 (a - b)^2
 *          (the numbering of the node2vec paper's table; fp32).  All four are symmetric: exchanging u and v changes no output bit.
 *   z_i  = w . x_i + b
 *   loss = (1/m) sum_i [softplus(z_i) - y_i z_i] + (l2 / 2) |w|^2                    (the bias is not regularised)
 *   gw   = (1/m) sum_i (sigmoid(z_i) - y_i) x_i + l2 w,   gb = (1/m) sum_i (sigmoid(z_i) - y_i)
 * in the stable forms of gg_classifier_ml_*: a logit of +-200 gives a finite loss and a term of exactly 0 - y or 1 - y; the loss
 * at zero parameters is log 2.
 * gg_edge_classifier_lossgrad: loss_out[1], gw_out[d], gb_out[1] at the given (w, b): ONE sweep over the edges (both rows of
 *   an edge are read once, as float4; 16 lanes per edge, the next edges' rows in flight while the current ones compute) and
 *   the reduction of gg_classifier_*.
 * gg_edge_classifier_fit: as gg_classifier_fit -- `iters` steps of full-batch Adam (0.9, 0.999, 1e-8, bias-corrected, step count
 *   from 1) on (w, b) from the values in w_inout / b_inout, which receive the result; loss_out[t] (may be NULL) is the loss
 *   BEFORE update t; one synchronisation at the end; ms_out (may be NULL): HIP-event time of the iterations.
 * gg_edge_classifier_predict: logits_out[i] = z_i, the bits the sweep computes for the same edge.
 * limits       op in [0, 3], n_emb <= 256, 1 <= m <= 2^31 - 1, node ids in [0, n_node), free to repeat, u[i] == v[i] is legal
 *              (the feature of a self-pair is well defined); y in {0, 1}; iters in [1, 10^6], lr > 0, finite l2 >= 0.  Anything
 *              else: GG_EINVAL, the gg_last_error text names the entry point and the offending entry, nothing is launched.
 * determinism  as gg_classifier_*: a grid that depends on m alone, every workgroup folds its lane groups in a fixed order and
 *              writes one partial to a stage, the stage is added in a fixed order; no floating-point atomics: the same inputs
 *              and table give the same bits. */
int gg_edge_classifier_lossgrad(gg_ctx *ctx, int which, int op, const int32_t *u, const int32_t *v, const int32_t *y /* 0 | 1 */, int64_t m,
                                const float *w, const float *b /* [1] */, float l2, float *loss_out, float *gw_out /* [d] */, float *gb_out /* [1] */);
int gg_edge_classifier_fit(gg_ctx *ctx, int which, int op, const int32_t *u, const int32_t *v, const int32_t *y, int64_t m, int iters,
                           float lr, float l2, float *w_inout, float *b_inout, float *loss_out /* [iters] or NULL */, double *ms_out);
int gg_edge_classifier_predict(gg_ctx *ctx, int which, int op, const int32_t *u, const int32_t *v, int64_t m, const float *w,
                               const float *b, float *logits_out /* [m] */);

/* ---- node clustering (additive entry points; GG_ABI_VERSION stays 9: no existing symbol, struct or behaviour changes).
 * Lloyd's k-means on the FROZEN rows of table `which` (0 = generator, 1 = discriminator), gathered by node id from the resident
 * table; nothing of size m x n_emb crosses to the host.  With d = n_emb, centroids fp32 [k, d] row-major, rows i = 0 .. m - 1:
 *   h_c     = |c_c|^2 / 2 (fp32, columns ascending),   g_ic = h_c - x_i . c_c,   x_i = E[nodes[i]]
 *   a_i     = argmin_{c < k} g_ic, TIES TO THE LOWEST CLUSTER INDEX; a row whose scores are all NaN gets cluster 0, and no index
 *             outside [0, k) is ever produced (non-finite tables are otherwise out of contract)
 *   dist2_i = max(0, |x_i|^2 + 2 g_{i, a_i}),   inertia = sum_i dist2_i (float64)
 *   sums[c] = sum_{a_i = c} x_i (fp32; the one-hot product only adds),   counts[c] = |{i : a_i = c}| (integers)
 * gg_kmeans_step: ONE sweep over the rows (every row is read once; both products on v_mfma_f32_32x32x2_f32) plus the reduction,
 *   at the given centroids.  Exactly one of `centroids` (values) and `centroid_nodes` (centroid c = row centroid_nodes[c] of the
 *   same table: the bits of both forms are equal) is non-NULL, else GG_EINVAL.  Every output may be NULL; with sums_out and
 *   counts_out both NULL the sweep skips the second product (the same assign, dist2 and inertia bits).
 * gg_kmeans_fit: sweep t = 1 .. max_iters assigns against C_t and gives a_t, sums, counts, inertia_t; inertia_out[t - 1] is
 *   written for the sweeps that ran, later entries are not.  After sweep t:
 *     1. t >= 2 and a_t == a_{t-1}:  stop, iters = t, converged = 1, C_t unchanged (a fixed point of the update);
 *     2. else t == max_iters:        stop, iters = t, converged = 0, NO update;
 *     3. else C_{t+1}[c] = sums[c] / (float)counts[c] (one IEEE fp32 division); an EMPTY cluster keeps its centroid bits.
 *   The returned centroids, assign, dist2, counts and last inertia are therefore mutually consistent: gg_kmeans_step at the
 *   returned centroids reproduces them bit for bit -- the fit's sweeps and reductions are the same kernels on the same grid.
 *   C_1 = centroids_inout, or with init_nodes the table rows init_nodes[c]; centroids_inout receives the result.  All
 *   max_iters iterations are enqueued behind one another, the stop is a device-side flag, one synchronisation at the end.
 *   ms_out (may be NULL): HIP-event time of the iterations.  assign_out, dist2_out, counts_out, inertia_out, iters_out,
 *   converged_out may be NULL.
 * limits       1 <= k <= 128, n_emb <= 256, 1 <= m <= 2^31 - 1, node ids (nodes, centroid_nodes, init_nodes) in [0, n_node),
 *              free to repeat; m < k is legal (clusters stay empty); max_iters in [1, 10^6].  Anything else: GG_EINVAL, the
 *              gg_last_error text names the limit, nothing is launched.
 * determinism  as gg_classifier_*: a grid that depends on m alone, every workgroup writes its partials to a stage, a second
 *              kernel adds the stage in a fixed order; no floating-point atomics: the same inputs and table give the same bits. */
int gg_kmeans_step(gg_ctx *ctx, int which, const int32_t *nodes, int64_t m, int k, const float *centroids /* [k * d] or NULL */,
                   const int32_t *centroid_nodes /* [k] or NULL */, int32_t *assign_out /* [m] or NULL */, float *dist2_out /* [m] or NULL */,
                   float *sums_out /* [k * d] or NULL */, int32_t *counts_out /* [k] or NULL */, double *inertia_out /* [1] or NULL */);
int gg_kmeans_fit(gg_ctx *ctx, int which, const int32_t *nodes, int64_t m, int k, int max_iters, float *centroids_inout /* [k * d] */,
                  const int32_t *init_nodes /* [k] or NULL */, int32_t *assign_out, float *dist2_out, int32_t *counts_out,
                  double *inertia_out /* [max_iters] or NULL */, int32_t *iters_out, int32_t *converged_out, double *ms_out);

/* ---- silhouette of a node partition (additive entry point; GG_ABI_VERSION stays 9: no existing symbol, struct or behaviour
 * changes).  The exact silhouette coefficient over ALL pairs of the FROZEN rows x_i = E[nodes[i]] of table `which` under the
 * partition c_i = assign[i] in [0, k), n_c = the size of cluster c; the label-free twin of the scores gg_kmeans_* is judged
 * by.  A consumer of the matrix-core tile stream (gg_all_score_reduce, gg_topk_scores, gg_rank_scores): nothing of size m x m
 * or m x n_emb crosses to the host.  For every evaluated position i, in fp32:
 *   dist_ij = sqrtf(max(0, (h_i + h_j) - 2 s_ij)), the square root correctly rounded;
 *             precision 0 (fp32): s_ij = the bits of gg_all_score's k-ordered fmaf chain of x_i . x_j, h_i = the same chain of
 *               row i with itself;
 *             precision 1 (bf16): s_ij = the bits of the bf16 stream (bf16 inputs, fp32 accumulate), h_i = the fp32 k-ordered
 *               fmaf chain over the bf16-ROUNDED row: the silhouette of the bf16-rounded table, as gg_rank_scores' bf16 leg;
 *   S_ic    = sum over j != i with c_j = c of dist_ij (fp32 sums in the implementation's fixed order); the own term is dropped
 *             BY POSITION, not by a computed distance of 0
 *   a_i     = S_{i, c_i} / (float)(n_{c_i} - 1)
 *   b_i     = min over c != c_i with n_c > 0 of S_ic / (float)n_c,   nearest_i = that c, TIES TO THE LOWEST c
 *   sil_i   = (b_i - a_i) / fmaxf(a_i, b_i);   n_{c_i} = 1: sil_i = 0 and a_i = 0 (the scikit-learn convention; b_i and nearest_i
 *             are still those above);   fmaxf(a_i, b_i) = 0: sil_i = 0
 *   mean    = (float64 sum of sil_i in output order) / count
 * rows == NULL evaluates every position (outputs [m], in the order of `nodes`); otherwise the positions rows[t] into `nodes`
 * (outputs [n_rows], entry t for rows[t]; a position MAY REPEAT, its entries are then equal), each against all m columns.
 * Every output may be NULL.  ms_out: HIP-event time of the device work (copy, stream passes, finish).
 * limits       2 <= k <= 128, 2 <= m <= 2^31 - 1, at least two non-empty clusters, node ids in [0, n_node) and DISTINCT, assign
 *              in [0, k), rows in [0, m) with 1 <= n_rows <= 2^31 - 1, precision 0 or 1; the widths of the tile stream (fp32
 *              n_emb <= 1116, bf16 n_emb <= 512).  Anything else: GG_EINVAL, the gg_last_error text names the limit, nothing
 *              is launched.
 * determinism  no floating-point atomics: the same inputs and table give the same bits.  The set is laid out sorted by
 *              (cluster, node id), every sum runs over that layout, and the column split depends on the set alone, so the
 *              outputs of a node do not depend on the order in which `nodes` lists the set (a permuted call returns the permuted
 *              outputs bit for bit), and with `rows` every entry equals the full call's entry bit for bit.
 * memory       the (row, cluster) stage is bounded by internal row passes of at most 4 096 rows (fewer for many clusters: at
 *              most 64 MiB); temporary device buffers are freed on every exit path. */
int gg_silhouette(gg_ctx *ctx, int which, const int32_t *nodes, const int32_t *assign, int64_t m, int k,
                  const int64_t *rows /* [n_rows] positions into nodes, or NULL = all */, int64_t n_rows, int precision /* 0 fp32, 1 bf16 */,
                  float *sil_out, float *a_out, float *b_out, int32_t *nearest_out /* each [n_rows or m] or NULL */,
                  double *mean_out /* [1] or NULL */, double *ms_out);

/* ---- centred Gram matrix of gathered rows (additive entry point; GG_ABI_VERSION stays 9: no existing symbol, struct or behaviour
 * changes).  The device part of the PCA of the FROZEN rows x_i = E[nodes[i]] of table `which` (0 = generator, 1 = discriminator):
 * nothing of size m x n_emb crosses to the host.  With d = n_emb, rows i = 0 .. m - 1:
 *   c_ij        = x_ij - center[j], ONE fp32 subtraction; center == NULL: c = x bit for bit (a NULL centre and an all-(+0) centre
 *                 give the same bits).  Rows behind m and columns behind d contribute exact zeros, never 0 - center.
 *   grid        = min(512, ceil(m / 64)) persistent workgroups over 64-row tiles, round robin (tile t belongs to workgroup
 *                 t mod grid): a function of m alone.
 *   part_w[j][l] = the k-ordered fmaf chain from 0.0 of c_ij c_il over the rows of workgroup w in ascending order (the arithmetic
 *                 of v_mfma_f32_32x32x2_f32);   psum_w[j] = the fp32 chain s = s + c_ij over the same rows.
 *   symmetry    only the tiles (a, b), a <= b, of the 32 x 32 output tiling are computed; the mirror is a copy:
 *                 gram[j][l] == gram[l][j] bit for bit.
 *   gram_out[j][l] = sum_w (double)part_w[j][l],   sums_out[j] = sum_w (double)psum_w[j]: float64, w ascending, by a second kernel.
 * gram_out == NULL takes a sums-only sweep (the mean pass: gather, subtract, add; no product), with the same sums bits.
 * Every output may be NULL.  ms_out: HIP-event time of the device work (sweep and reduction).
 * limits       n_emb <= 256, 1 <= m <= 2^31 - 1, node ids in [0, n_node), free to repeat, center finite.  Anything else:
 *              GG_EINVAL, the gg_last_error text names the entry point and the offending entry, nothing is launched.
 * determinism  no floating-point atomics: the same inputs and table give the same bits.
 * memory       the stage is grid x d x d floats (134 MB at 512 workgroups and d = 256); temporary device buffers are freed on
 *              every exit path. */
int gg_gram(gg_ctx *ctx, int which, const int32_t *nodes, int64_t m, const float *center /* [d] or NULL */,
            double *sums_out /* [d] or NULL */, double *gram_out /* [d * d] row-major or NULL */, double *ms_out);

/* ---- top-K under a metric and over a candidate set (additive entry point; GG_ABI_VERSION stays 9: no existing symbol, struct or
 * behaviour changes).  gg_topk_scores' retrieval -- the same tile stream, k-lists and merge -- ordered by cosine similarity or
 * Euclidean distance instead of the raw dot product, optionally restricted to a set of candidate nodes: "which nodes are most
 * similar to this one", and the neighbour query of a k-NN classifier.  For each requested node u (rows == NULL: every node,
 * n_rows ignored; repeated rows allowed) and table E of model `which`, every operation in fp32, in this order:
 *   s(u, c)     the bits the tile stream of `precision` gives for row u, column c, exactly as in gg_topk_scores;
 *   h_c         |x_c|^2: the k-ordered fmaf chain from 0.0 of row c with itself (precision 1: over the bf16-ROUNDED row, as in
 *               gg_silhouette), computed for all n_node columns once per call, in front of the passes;
 *   metric 0    (dot)     t = s;                                     reported score t.  With cand_nodes == NULL and exclude in
 *               {0, 1} every output bit equals gg_topk_scores';
 *   metric 1    (cosine)  w_c = 1.0f / sqrtf(h_c) (a correctly rounded square root, one IEEE division; w_c = 0 where h_c == 0);
 *               t = s * w_c, ONE multiply;                           reported score t * w_u, ONE multiply where the merged list is
 *               written out.  A zero row or a zero column scores 0;
 *   metric 2    (l2)      t = fmaf(-0.5f, h_c, s);                   reported value the SQUARED distance
 *               fmaxf(0.f, fmaf(-2.f, t, h_u)).  The list is NEAREST FIRST;
 *   order       t descending, column ascending, -0 counting as +0 (the key ord(t) << 32 | ~col of gg_topk_scores).  The reported
 *               value is a monotone image of t under a single rounding (w_u >= 0; -2 < 0), so every returned list is
 *               non-increasing (dot, cosine) or non-decreasing (l2); columns with equal t stand in ascending order, also where
 *               their reported values are equal;
 *   eligible    the AND of two conditions.  exclude = 0: every node; 1: not u and not u's neighbours in the resident training
 *               graph (gg_set_graph_csr; without a graph: GG_EINVAL); 2: not u itself (needs no graph).  cand_nodes != NULL: only
 *               the n_cand listed nodes (ids in [0, n_node), free to repeat; n_cand = 0: nothing is eligible); the library turns
 *               the ids into an n_node-bit bitmap on the device.  Like the adjacency, the bit is read only where a column is about
 *               to enter a list: an ineligible column never enters one and never raises a list's threshold;
 *   result      out_col[n_rows][k] (int32) and out_score[n_rows][k] (fp32), row-major; a row with fewer than k eligible columns
 *               is padded with col -1 and score -inf (metric 2: +inf).
 * limits       1 <= k <= 256, metric in {0, 1, 2}, exclude in {0, 1, 2}, precision 0 or 1, n_cand >= 0, the widths of the tile
 *              stream (fp32 n_emb <= 1116, bf16 n_emb <= 512), ids in [0, n_node).  Anything else: GG_EINVAL, the gg_last_error
 *              text names gg_topk_metric and the limit (for an id: the array and the FIRST bad index), nothing is launched.
 *              Non-finite values: unspecified.
 * determinism  no atomics: the same inputs and table give the same bits.  A row's outputs depend on the row, the set and k alone.
 * kernel_ms_out (may be NULL): HIP-event time of the norm pass, the tile streams and the merges (the bf16 copy excluded, as in
 * gg_topk_scores).  Temporary device buffers are freed on every exit path. */
int gg_topk_metric(gg_ctx *ctx, int32_t which, const int32_t *rows, int32_t n_rows, int32_t k, int32_t precision, int32_t metric,
                   int32_t exclude, const int32_t *cand_nodes, int64_t n_cand, int32_t *out_col, float *out_score, double *kernel_ms_out);

/* ---- pair-neighbour sweep (additive entry points; GG_ABI_VERSION stays 9: no existing symbol, struct or behaviour changes).
 * The device part of the neighbourhood link-prediction indices -- common neighbours, Jaccard, Adamic-Adar, resource allocation,
 * preferential attachment -- on the resident training graph (gg_set_graph_csr).  No embedding table is read.
 *   N(x)        the neighbour SET of node x: the distinct entries of x's resident list other than x itself (the resident lists
 *               keep duplicates and list a self-loop twice; the sets do not);
 *   deg(x)      |N(x)|;
 *   C(u, v)     (N(u) & N(v)) \ {u, v}; u == v is allowed and follows the formulas: C(u, u) = N(u).
 * gg_distinct_degrees: deg[x] = deg(x) for every node.
 * gg_pair_neighbors, for the pairs i = 0 .. m - 1:
 *   cn[i]       = |C(u_i, v_i)|,   deg_u[i] = deg(u_i),   deg_v[i] = deg(v_i);
 *   wsum[j * m + i] = sum over w in C(u_i, v_i) of weights[j * n_node + w],  j = 0 .. n_w - 1: a sum of UNSIGNED 64-BIT INTEGERS --
 *               exact, independent of the order of the terms and of how the work was split.  Fixed-point node weights make the
 *               result a bit contract without prescribing a reduction shape: exchanging u and v, permuting the pairs, running
 *               again or splitting one pair over several wavefronts changes no bit.
 * The sets are kept as an adjacency of their own (sorted lists under int64 row offsets), built on the host on first use after
 * gg_set_graph_csr, which drops it.  A group of 4, 16 or 64 lanes per pair -- chosen from the pair's shorter list -- walks that
 * list and looks each entry up in the longer one by binary search; a pair whose shorter list is longer than 512 entries is
 * split into tasks of 512 entries that add into the zeroed outputs with integer atomics.
 * limits       0 <= n_w <= 4; m >= 0 (m == 0 succeeds and writes nothing); ids in [0, n_node); cn, deg_u and deg_v not NULL;
 *              weights and wsum not NULL when n_w > 0 (ignored when n_w == 0); max(weights) * max(deg) must fit in 63 bits
 *              (checked on the host, so no sum can wrap); a resident graph.  Anything else: GG_EINVAL, the gg_last_error text
 *              names the entry point (for an id: the array and the FIRST bad index), nothing is launched.
 * determinism  integer arithmetic only: the same inputs give the same bits.
 * weights are uploaded by every call.  kernel_ms (may be NULL): HIP-event time of the sweep kernels on the context's stream.
 * Temporary device buffers are freed on every exit path. */
int gg_distinct_degrees(gg_ctx *ctx, int32_t *deg /* [n_node] */);
int gg_pair_neighbors(gg_ctx *ctx, const int32_t *u, const int32_t *v, int64_t m,
                      const uint64_t *weights /* [n_w * n_node] or NULL */, int32_t n_w /* 0 .. 4 */,
                      int32_t *cn /* [m] */, int32_t *deg_u /* [m] */, int32_t *deg_v /* [m] */,
                      uint64_t *wsum /* [n_w * m] or NULL when n_w == 0 */, double *kernel_ms /* or NULL */);

/* ---- neighbour-sum sweep (additive entry points; GG_ABI_VERSION stays 9: no existing symbol, struct or behaviour changes).
 * A CSR times dense-matrix product on the set adjacency N(v) of the resident training graph -- the one gg_pair_neighbors uses
 * (sorted, distinct, without the node itself) -- and label spreading (Zhou et al. 2004) iterated on it.  Needs gg_set_graph_csr;
 * no embedding table is read.
 *
 * gg_neighbor_sum: X fp32 [n_node, n_col], in_scale / out_scale fp32 [n_node] or NULL, nodes int32 [m] or NULL for all nodes
 * (m is then not read and out is [n_node, n_col]); with v = nodes[i]
 *   out[i, c] = out_scale[v] * sum over w in N(v) of (in_scale[w] * X[w, c]).
 * NULL means "no multiply" (the bits equal those of a scale of 1.0f).
 *   arithmetic  one separately rounded fp32 multiply per gathered element where in_scale is given, fp32 adds, one separately
 *               rounded fp32 multiply at the end where out_scale is given; no fused multiply-add.  A node without neighbours
 *               gives +0.
 *   bit contract  the ORDER of a node's adds is not specified.  The bits of out for node v are a function of N(v), the gathered
 *               rows, the scales and n_col alone: they do not depend on which other nodes were requested, on their order, on the
 *               grid or on the run.  A rerun, a permuted `nodes`, a subset and a repeated id return the same bits per node; there
 *               are no floating-point atomics.  Where every partial sum is exactly representable (integer inputs with sums below
 *               2^24) the result is exact.
 *   shape       rows are padded on the device to CP = 4 ceil(n_col / 4) floats; a row takes LPR lanes, the smallest power of two
 *               >= CP / 4; a wavefront works on one node, its 64 / LPR lane groups each on a different neighbour, four rows in
 *               flight per group, folded by a fixed shuffle tree.  A node with more than 512 neighbours is split into tasks of
 *               512 entries that write partial rows into a stage; a finishing kernel adds a node's partial rows in ascending
 *               chunk order.  The split depends on the node's degree alone.  The task plan of the all-nodes sweep is built once
 *               per graph and dropped by gg_set_graph_csr.
 *   limits      1 <= n_col <= 128; m >= 0 (m == 0 succeeds and writes nothing); X and out not NULL; ids in [0, n_node); a
 *               resident graph.  Anything else: GG_EINVAL, the gg_last_error text names the entry point and the value (for an
 *               id: the FIRST bad index), nothing is launched.
 *
 * gg_label_spread: F <- alpha S F + (1 - alpha) Y, S = D^-1/2 A D^-1/2 on N, from F_0 = Y0 for `iters` iterations.
 *   train_nodes int32 [m_train] distinct; label_bits uint32 [m_train, ceil(n_class / 32)]: bit c & 31 of word c >> 5 says that
 *   the node has label c (one bit: single label; several: multi-label); Y0[v, c] = 1 for those, else 0.
 *   s, a        fp32 [n_node]: s[v] = fp32(1 / sqrt(deg(v))), a[v] = fp32(alpha / sqrt(deg(v))), 0 where deg(v) = 0, as the caller
 *               rounded them (one host function serves the device and the host path); b = fp32(1 - alpha), float64 subtraction.
 *   iteration   H = neighbor_sum(F_t, in_scale = s);  F_{t+1}[v, c] = (a[v] * H[v, c]) + (Y0[v, c] ? b : 0): two separately rounded
 *               fp32 operations, no fused multiply-add.  The fit and gg_neighbor_sum run ONE sweep kernel (the epilogue is a
 *               compile-time variant), so gg_label_spread(iters = T) equals T calls of gg_neighbor_sum composed on the host with
 *               float32 a * H + base, bit for bit.
 *   outputs     F_out[i, :] = F_T[out_nodes[i], :] (out_nodes NULL: every node, m_out is then not read); *delta =
 *               max |F_T - F_{T-1}| over all n_node x n_class entries (fp32 subtraction; an integer maximum of non-negative float
 *               bits on the device, so order-independent).  m_out == 0 runs the fit, writes no row and returns delta.
 *   residency   F_t, F_{t+1} and the label masks of all nodes live on the device for the whole call; Y0 is built there from the
 *               masks; the plan is not rebuilt or uploaded per iteration.  Nothing of size n_node x n_class crosses to the host
 *               except F_out when out_nodes is NULL.
 *   limits      1 <= n_class <= 128; m_train >= 0; m_out >= 0; train_nodes, label_bits, s, a not NULL; F_out not NULL when rows
 *               are asked for; 0 < alpha < 1; iters >= 1; ids in [0, n_node); no repeated training node; no label bit at or above
 *               n_class.  Anything else: GG_EINVAL as above.
 * kernel_ms (may be NULL): HIP-event time of the sweep kernels (of all iterations) on the context's stream; uploads, the Y0
 * kernel and the read-back are outside.  Temporary device buffers are freed on every exit path. */
int gg_neighbor_sum(gg_ctx *ctx, const float *X /* [n_node, n_col] */, int32_t n_col, const float *in_scale /* [n_node] or NULL */,
                    const float *out_scale /* [n_node] or NULL */, const int32_t *nodes /* [m] or NULL */, int64_t m,
                    float *out /* [m, n_col] */, double *kernel_ms /* or NULL */);
int gg_label_spread(gg_ctx *ctx, const int32_t *train_nodes /* [m_train] */, const uint32_t *label_bits, int64_t m_train, int32_t n_class,
                    double alpha, int32_t iters, const float *s /* [n_node] */, const float *a /* [n_node] */,
                    const int32_t *out_nodes /* [m_out] or NULL */, int64_t m_out, float *F_out /* [m_out, n_class] */,
                    float *delta /* or NULL */, double *kernel_ms /* or NULL */);

/* ---- neighbour-mode sweep (additive entry points; GG_ABI_VERSION stays 9: no existing symbol, struct or behaviour changes).
 * The most frequent neighbour label of every node -- the step of label-propagation community detection (Raghavan et al. 2007) --
 * the propagation iterated on the device, and the edge counts of a partition from which modularity is one float64 formula.  All
 * on the set adjacency of the resident training graph: N(v) and deg(v) are those of the pair-neighbour sweep (distinct entries,
 * no self-loop).  Needs gg_set_graph_csr; no embedding table is read; every result is an integer.
 *   fmix32      the MurmurHash3 finaliser on uint32, all arithmetic mod 2^32:
 *               x ^= x >> 16;  x *= 0x85ebca6b;  x ^= x >> 13;  x *= 0xc2b2ae35;  x ^= x >> 16.
 *
 * gg_neighbor_mode: labels int32 [n_node], every one >= 0; nodes int32 [m] or NULL for all nodes (m is then not read and out is
 * [n_node]); with v = nodes[i], cnt(l) = |{w in N(v) : labels[w] == l}| and cmax = max over l of cnt(l):
 *   deg(v) == 0                          out[i] = labels[v];
 *   keep != 0 and cnt(labels[v]) == cmax   out[i] = labels[v];
 *   otherwise                            out[i] = the label l with cnt(l) == cmax that has the smallest pair (fmix32(l ^ salt), l).
 *   bit contract  integers only and a total order: out for node v is a function of N(v), the labels, salt and keep alone.  A
 *               rerun, a permuted or repeated `nodes` and a subset return the same value per node.
 *   shape       by deg(v): up to 64, a group of 4, 16 or 64 lanes (one neighbour per lane, the equal labels counted by broadcast
 *               and compare, the triples (count descending, hash ascending, label ascending) folded by a shuffle tree); up to
 *               2048, one workgroup with an open-addressing (label, count) table in LDS of the power of two >= 2 deg(v) slots,
 *               claimed by compare-and-swap and counted by integer adds; above, the same on a zeroed table in global memory from
 *               a scratch buffer of the context.  No list is truncated; no path depends on the number of distinct labels.  The
 *               task plan of the all-nodes sweep is built once per graph and dropped by gg_set_graph_csr.
 *   limits      m >= 0 (m == 0 succeeds and writes nothing); labels and out not NULL; labels >= 0; ids in [0, n_node); a resident
 *               graph.  Anything else: GG_EINVAL with the texts
 *                 "gg_neighbor_mode: needs the training graph (gg_set_graph_csr)", "gg_neighbor_mode: m = <m> is negative",
 *                 "gg_neighbor_mode: labels and out must not be NULL", "gg_neighbor_mode: labels[<v>] = <l> is negative" (the FIRST
 *                 offender), "gg_neighbor_mode: nodes[<i>] = <id> out of range [0, <n_node>)" (the FIRST bad index);
 *               nothing is launched.
 *
 * gg_label_propagation: from L[v] = v, iterations t = 1, 2, ...:
 *   st = fmix32((seed ^ 0x85ebca6b) + 0x9E3779B9 * t),   side(v) = fmix32(v ^ st) & 1;
 *   half-step h = 0, then h = 1: the nodes with side(v) == h take gg_neighbor_mode(L, salt = fmix32(seed + 0x9E3779B9 *
 *   (2 (t - 1) + h + 1)), keep = 1) all at once, every other node keeps its label;
 *   changed[t - 1] = the number of labels the two half-steps moved; stop at the first t with changed == 0 (*converged = 1) or
 *   after max_iters (*converged = 0); *iters = t, labels = L.  The split is redrawn every iteration: with a fixed split pairs of
 *   nodes on one side keep swapping labels for ever.
 *   residency   L, the side test and the changed words stay on the device for the whole call; one 4-byte count per iteration
 *               crosses to the host.  The half-steps run the kernels of gg_neighbor_mode (the side is an argument), so T
 *               iterations equal 2 T calls of gg_neighbor_mode composed on the host, bit for bit.
 *   limits      max_iters >= 1 ("gg_label_propagation: max_iters = <k> is below 1"); labels, iters, converged and changed
 *               (int32 [max_iters]; entries behind *iters are not written) not NULL ("gg_label_propagation: labels, iters,
 *               converged and changed must not be NULL"); a resident graph ("gg_label_propagation: needs the training graph
 *               (gg_set_graph_csr)").
 *
 * gg_partition_edges: assign int32 [n_node], assign[v] in [0, n_label) or -1 for "outside the partition";
 *   tot[c]   = sum over v with assign[v] == c of |{w in N(v) : assign[w] >= 0}|,
 *   intra[c] = sum over v with assign[v] == c of |{w in N(v) : assign[w] == c}|   (ordered pairs: an inner edge counts twice).
 *   With M2 = sum of tot, modularity is Q = sum over c of (intra[c] / M2 - (tot[c] / M2)^2) -- computed by the caller in float64.
 *   shape       groups of 4, 16 or 64 lanes per node (deg <= 8, <= 64, above), a list longer than 512 entries split into tasks
 *               of 512.  A group's first lane holds the counts of its tasks while their class stays the same, and the lanes of a
 *               wavefront that add into one class add through one lane: unsigned 64-bit atomic adds, exact whatever the order,
 *               and few of them where the partition has few classes.
 *   limits      n_label >= 1 ("gg_partition_edges: n_label = <k> is below 1"); assign, intra and tot not NULL
 *               ("gg_partition_edges: assign, intra and tot must not be NULL"); "gg_partition_edges: assign[<v>] = <a> outside
 *               [-1, <n_label>)" (the FIRST offender); "gg_partition_edges: needs the training graph (gg_set_graph_csr)".
 * kernel_ms (may be NULL): HIP-event time on the context's stream -- of the sweep kernels (gg_neighbor_mode, gg_partition_edges)
 * or of the whole fit with its per-iteration read-backs (gg_label_propagation).  Temporary device buffers are freed on every
 * exit path. */
int gg_neighbor_mode(gg_ctx *ctx, const int32_t *labels /* [n_node] */, uint32_t salt, int32_t keep, const int32_t *nodes /* [m] or NULL */,
                     int64_t m, int32_t *out /* [m] */, double *kernel_ms /* or NULL */);
int gg_label_propagation(gg_ctx *ctx, uint32_t seed, int32_t max_iters, int32_t *labels /* [n_node] */, int32_t *iters, int32_t *converged,
                         int32_t *changed /* [max_iters] */, double *kernel_ms /* or NULL */);
int gg_partition_edges(gg_ctx *ctx, const int32_t *assign /* [n_node] */, int32_t n_label, int64_t *intra /* [n_label] */,
                       int64_t *tot /* [n_label] */, double *kernel_ms /* or NULL */);

/* ---- two-hop sweep (additive entry points; GG_ABI_VERSION stays 9: no existing symbol, struct or behaviour changes).
 * Per query node u one row of A W A on the set adjacency of the resident training graph -- N(x) and deg(x) are those of the
 * pair-neighbour sweep (distinct entries, no self-loop) -- and from it the best k candidates or the place of one target: the
 * graph-only baseline of the ranking evaluators (gg_topk_scores / gg_rank_scores on the embedding side), and "friends of friends"
 * recommendation from an edge list.  Needs gg_set_graph_csr; no embedding table is read; every result is an integer.
 *   score       S(u, c) = sum over w in N(u) & N(c) of weights[w], unsigned 64-bit; weights uint64 [n_node] or NULL = every weight
 *               1 (common neighbours).  S(u, c) equals the cn / wsum of gg_pair_neighbors for the pair (u, c), also at c == u,
 *               where S = the sum over N(u).  max(weights) * max(deg) must fit in 63 bits (checked on the host).
 *   eligibility exclude = 1 ("self"): every c != u;  exclude = 2 ("graph"): every c outside N(u) + {u} -- the candidates of
 *               gg_topk_scores with exclude = 1.
 *   order       score descending, column ascending (the order of gg_topk_scores / gg_rank_scores).
 *
 * gg_two_hop_topk: rows int32 [n_rows], ids may repeat; 1 <= k <= 256.  Row i of out_col / out_score [n_rows, k] gets the first k
 * eligible candidates with S > 0 in that order, padded with col = -1, score = 0; n_pos[i] = the number of eligible candidates with
 * S > 0 (it may exceed k).  Zero-score nodes never enter a list: they would fill it by node id.
 *
 * gg_two_hop_rank: queries (u[i], v[i]), i < m.  The target v is always a candidate, also where the exclusion rule would drop it
 * (the contract of gg_rank_scores).  Over the eligible c != v:
 *   score[i]     = S(u, v);
 *   n_pos[i]     = |{c : S(u, c) > 0}|;
 *   ahead[i]     = |{c : S(u, c) > 0 and (S(u, c) > S(u, v) or (S(u, c) == S(u, v) and c < v))}|;
 *   pos_below[i] = |{c : S(u, c) > 0 and c < v}|.
 * The position of v among ALL its candidates follows on the host (graphgan_amd/evaluation/graph_ranking.py: full_rank, the one
 * function of the device and the host path): rank = 1 + ahead if score > 0, else 1 + n_pos + (E_below - pos_below), E_below = the
 * eligible c < v = v minus the ids below v in excl(u) \ {v}; n_cand = n_node - |excl(u) \ {v}|.  The zero-score nodes are never
 * visited.  With an eligible target and score > 0, rank <= k holds exactly when gg_two_hop_topk lists v at position rank - 1 with
 * the same score.
 *
 *   bit contract  integers only and a total order: a query's outputs are a function of the graph, the weights, exclude and the
 *               query alone.  A rerun, permuted, repeated or subset queries and any scratch_bytes return the same bits per query.
 *   shape       the host plans per query T(u) = sum over w in N(u) of deg(w), the entries of the expansion.  One workgroup per
 *               query fills an open-addressing (column, uint64 sum) table of the power of two >= 2 min(T, n_node) slots (at least
 *               256): slots claimed by compare-and-swap, values added with 64-bit integer atomics, linear probing from column mod
 *               slots.  T <= 2048: the table lies in LDS; above, in a zeroed table of a scratch buffer of the context.  Lists
 *               N(w) of up to 64 entries are walked by groups of 16 lanes, longer ones by the whole workgroup: no list is
 *               truncated.  Then one scan of the table: for the rank, counts by compares against the target's entry; for the
 *               lists, a radix select on the composite key (score, ~column), 8 bits per pass, and a bitonic sort of the
 *               survivors.  Eligibility under exclude = 2 is a binary search in the sorted N(u).
 *   scratch_bytes  the cap on the global-memory tables of one internal pass; 0 = the default (256 MiB).  Queries whose tables do
 *               not fit together run in several passes; a pass holds at least one query whatever its table's size.
 *   limits      n_rows, m >= 0 (0 succeeds and writes nothing) and below 2^31; ids in [0, n_node); a resident graph.  Anything
 *               else: GG_EINVAL with the texts (<fn> = the entry point's name, <m> = "n_rows" or "m")
 *                 "<fn>: needs the training graph (gg_set_graph_csr)", "<fn>: <m> = <value> is negative",
 *                 "<fn>: <m> = <value> does not fit in 31 bits", "<fn>: exclude = <e> is neither 1 (self) nor 2 (graph)",
 *                 "<fn>: scratch_bytes = <b> is negative", "gg_two_hop_topk: k = <k> outside [1, 256]",
 *                 "gg_two_hop_topk: rows, out_col, out_score and n_pos must not be NULL",
 *                 "gg_two_hop_rank: u, v, score, ahead, n_pos and pos_below must not be NULL",
 *                 "<fn>: rows[<i>] = <id> out of range [0, <n_node>)" (likewise u, then v; the FIRST bad index),
 *                 "<fn>: the largest weight <w> times the largest degree <d> does not fit in 63 bits";
 *               nothing is launched.
 * kernel_ms (may be NULL): HIP-event time of the sweep kernels and the table clears on the context's stream, summed over the
 * internal passes.  Temporary device buffers are freed on every exit path. */
int gg_two_hop_topk(gg_ctx *ctx, const int32_t *rows /* [n_rows] */, int64_t n_rows, int32_t k, const uint64_t *weights /* [n_node] or NULL */,
                    int32_t exclude, int64_t scratch_bytes, int32_t *out_col /* [n_rows, k] */, uint64_t *out_score /* [n_rows, k] */,
                    int32_t *n_pos /* [n_rows] */, double *kernel_ms /* or NULL */);
int gg_two_hop_rank(gg_ctx *ctx, const int32_t *u /* [m] */, const int32_t *v /* [m] */, int64_t m, const uint64_t *weights /* [n_node] or NULL */,
                    int32_t exclude, int64_t scratch_bytes, uint64_t *score /* [m] */, int32_t *ahead /* [m] */, int32_t *n_pos /* [m] */,
                    int32_t *pos_below /* [m] */, double *kernel_ms /* or NULL */);

/* ---- two-hop pair sweep (additive entry point; GG_ABI_VERSION stays 9: no existing symbol, struct or behaviour changes).
 * gg_two_hop_top_pairs: the k best pairs of the WHOLE node set by a neighbourhood index -- "the k most likely missing edges from an
 * edge list alone" -- the graph-only line beside gg_top_pairs.  On the neighbour SETS N(x) of the resident training graph (the set
 * adjacency of the two-hop sweep above: distinct entries, no self-loop).  Needs gg_set_graph_csr; no embedding table is read;
 * every result is an integer.
 *   score       S(u, v) = sum over w in N(u) & N(v) of weights[w], unsigned 64-bit; weights uint64 [n_node] or NULL = every weight
 *               1.  The value gg_pair_neighbors and gg_two_hop_rank report for (u, v).  w ranges over the WHOLE graph; only the
 *               endpoints are restricted by `nodes`.  max(weights) * max(deg) must fit in 63 bits (checked on the host).
 *   candidates  the unordered pairs {u, v}, u < v, both in `nodes` (NULL = every node, m is not read; otherwise m ids, STRICTLY
 *               ascending, m may be 0), with S(u, v) > 0 and, with exclude = 1, v not in N(u).  exclude = 0 keeps the edges: u < v
 *               rules out the self pair, so nothing has to be refused.  Zero-score pairs never enter: they would fill the list by id.
 *   order       score descending, then (u, v) ascending: total and integer.
 *   results     out_u, out_v int32 [k], out_score uint64 [k]: the first k (1 <= k <= 2^20) candidates in that order; *n_found =
 *               min(k, candidates); the entries behind n_found are -1, -1, 0.
 *               stats (int64 [6] or NULL) = {launches (batches of sources, one read-back each), retries, compactions, entries
 *               appended, sources swept, sources skipped by the bound}.  kernel_ms (or NULL): HIP-event time of the whole sweep on
 *               the context's stream, with its table clears, read-backs and compactions.
 *   bit contract  out_u, out_v, out_score and n_found are a function of the graph, the weights, nodes, k and exclude alone -- not of
 *               buffer_entries, scratch_bytes, the grid, the source order, the batches or the run.
 *   shape       One workgroup of 256 threads per source u.  Fill: the expansion of u restricted to the upper triangle -- for w in
 *               N(u) the suffix of the sorted N(w) above u, found by one binary search per list -- into the two-hop sweep's
 *               open-addressing (column, uint64 sum) table; the host plans the table from T'(u) = sum over w in N(u) of |{c in
 *               N(w), c > u}|, computed exactly: T' <= 2048 the table lies in LDS, above in a zeroed table of the context's
 *               scratch, the sources batched under scratch_bytes (0 = the default, 256 MiB; a pass holds at least one source).
 *               Lists of up to 64 entries are walked by groups of 16 lanes, longer ones by the workgroup.  Consume: ONE floor
 *               (fs 64 bits, fu, fv) in device memory, the k-th best pair known -- (0, max, max) until k are known -- read once
 *               per kernel; one scan of the table keeps the entries (c, x) with x > 0, c > u, the set's bit of c, c outside N(u)
 *               under exclude, and (x, u, c) strictly ahead of the floor, and appends them as (score lo, score hi, u, v) to a
 *               buffer with ONE integer atomic per wavefront and scan step on the fill counter -- it counts on past the capacity,
 *               the stores do not.  Host: the sources with T' > 0 go in descending B(u) = sum over w in N(u) of weights[w] (deg(u)
 *               without weights), ties by id; S(u, .) <= B(u), so a source with B(u) < fs is not launched (counted in stats).  A
 *               launch is a batch of consecutive sources, 256 at first, doubling to 65 536 while nothing overflows; one 4-byte
 *               read-back per launch; on overflow the counter is set back, the buffer compacted if it holds more than k entries
 *               and the batch rerun as two halves.  A compaction (on the host; when the fill passes min(k + (buffer_entries - k) /
 *               2, max(3 k, 2^16)), and at the end, where the k best are sorted) keeps the k best and stores the k-th as the floor.
 *   buffer_entries  0 = the default max(minimum, 2^22, 4 k), else in [minimum, max(2^26, minimum)], minimum = k + the largest
 *               min(T'(u), members above u): one source always fits behind k entries.
 *   limits      GG_EINVAL, nothing is launched, the text names gg_two_hop_top_pairs: "needs the training graph (gg_set_graph_csr)",
 *               "k = <k> outside [1, 2^20]", "exclude = <e> is neither 0 nor 1", "scratch_bytes = <b> is negative",
 *               "buffer_entries = <b> is negative", "out_u, out_v, out_score and n_found must not be NULL", "m = <m> is negative",
 *               "nodes[<i>] = <id> out of range [0, <n>)", "nodes[<i>] = <id> is not above nodes[<i - 1>] = <id> (strictly
 *               ascending ids)" (the FIRST bad index), "the largest weight <w> times the largest degree <d> does not fit in 63
 *               bits", "buffer_entries = <b> outside [<minimum>, <maximum>] (0: the default; the minimum is k + <bound>, the most
 *               entries one source can append)".  GG_ECAPACITY, nothing is launched: "one source reaches <e> nodes above it, more
 *               than 2^30: its table has no 32-bit slot count" (min(T'(u), n_node - 1 - u) > 2^30), "one source can append <b>
 *               entries: a buffer of more than 2^31 entries".  Temporary device buffers are freed on every exit path. */
int gg_two_hop_top_pairs(gg_ctx *ctx, const int32_t *nodes /* [m] or NULL */, int64_t m, int64_t k, const uint64_t *weights /* [n_node] or NULL */,
                         int32_t exclude, int64_t scratch_bytes, int64_t buffer_entries, int32_t *out_u /* [k] */, int32_t *out_v /* [k] */,
                         uint64_t *out_score /* [k] */, int64_t *n_found, int64_t *stats /* [6] or NULL */, double *kernel_ms /* or NULL */);

/* ---- push sweep (additive entry points; GG_ABI_VERSION stays 9: no existing symbol, struct or behaviour changes).
 * Per query node u the rooted (personalised) PageRank of u on the set adjacency of the resident training graph -- N(x) and deg(x)
 * are those of the pair-neighbour sweep (distinct entries, no self-loop) -- by the local push of Andersen, Chung & Lang, done
 * synchronously in fixed-point integers, and from it the best k candidates or the place of one target: the graph-only baseline of
 * the ranking evaluators that looks further than the two-hop sweep's two hops.  Needs gg_set_graph_csr; no embedding table is read;
 * every result is an integer.  ONE = 2^40.
 *   parameters  alpha_q in [1, 65535]: the restart probability in units of 2^-16;  eps_q in [1, 2^32]: the push threshold per unit
 *               of degree, in units of 2^-40 of the mass;  alpha_q * eps_q >= 65536, so that kmin = (eps_q * alpha_q) >> 16 >= 1;
 *               max_rounds >= 1.  With these ranges no product below reaches 2^63.
 *   state       p[x] and r[x], unsigned 64-bit, all zero except r[u] = ONE.
 *   a round     1. the active set is A = {x : r[x] > 0 and r[x] >= eps_q * max(deg(x), 1)};
 *               2. if A is empty the query has converged and stops;
 *               3. otherwise every x in A pushes simultaneously from its value r0 = r[x] at the START of the round:
 *                    keep  = (r0 * alpha_q) >> 16, or keep = r0 where deg(x) = 0 (only the root can be such a node);
 *                    rest  = r0 - keep;   share = rest / deg(x), integer division (0 for deg(x) = 0);   rem = rest - share * deg(x);
 *                    p[x] += keep;   r[x] = rem + (what arrives this round);   r[w] += share for every w in N(x);
 *               4. after max_rounds rounds the query stops unconverged.
 *   outputs     the score S(u, c) = p[c];  rounds = the rounds that pushed;  converged = 1 if the active set after the last round
 *               is empty;  residual = sum r.
 *   invariants  sum p + sum r == ONE after every round.  Every push of x retires keep >= deg(x) * kmin, so over a whole query the
 *               sum of deg(x) over all pushes is at most B = ONE / kmin, and at most E = min(n_node, 1 + B) distinct nodes are ever
 *               touched.  rem < deg(x) <= eps_q * deg(x): a node that pushed is inactive until something arrives.
 *   eligibility, order   those of the two-hop sweep: exclude = 1 ("self") or 2 ("graph"); score descending, column ascending;
 *               zero-score nodes never enter a list.
 *
 * gg_ppr_topk: rows int32 [n_rows], ids may repeat; 1 <= k <= 256.  out_col / out_score / n_pos as gg_two_hop_topk's with S = p.
 * gg_ppr_rank: queries (u[i], v[i]), i < m; score / ahead / n_pos / pos_below as gg_two_hop_rank's with S = p, and the rank follows
 * on the host by the same full_rank.  Queries with equal u that stand next to each other in the request share one push and scan
 * once per target; a query's outputs depend on its own (u, v) alone.
 * Both: rounds int32, converged int32 and residual uint64, one per query.
 *
 *   bit contract  all adds are integer and the pushes of a round read start-of-round values only: a query's outputs are a function
 *               of the graph, the parameters, exclude and the query alone.  A rerun, permuted, repeated or subset queries and any
 *               scratch_bytes return the same bits per query.
 *   shape       one workgroup of 256 threads per root.  One key array and two value arrays (r, p) over the slots of an
 *               open-addressing table of set_table_slots(E) slots (the power of two >= max(256, 2 E)), the frontier as a list.
 *               E <= 1024: everything lies in LDS; above, in zeroed scratch of the context.  Phase A: one thread per frontier
 *               entry computes keep / share / rem.  Phase B: lists of up to 64 entries are walked by groups of 16 lanes, longer ones
 *               by the whole workgroup; r[w] += share is a claim by compare-and-swap and a 64-bit integer atomic add whose returned
 *               old value tells the one adder that crosses the threshold to append w to the next frontier.  The round count and
 *               the frontier length stay on the device.  Then the two-hop sweep's consumers on (key, p).
 *   scratch_bytes  the cap on the global-memory tables of one internal pass; 0 = the default (2 GiB).  A pass holds at least one
 *               root whatever its tables' size.
 *   limits      those of the two-hop sweep with its texts under the new names ("gg_ppr_topk: k = <k> outside [1, 256]",
 *               "gg_ppr_topk: rows, out_col, out_score, n_pos, rounds, converged and residual must not be NULL",
 *               "gg_ppr_rank: u, v, score, ahead, n_pos, pos_below, rounds, converged and residual must not be NULL"), and
 *                 "<fn>: alpha_q = <a> outside [1, 65535]", "<fn>: eps_q = <e> outside [1, 4294967296]",
 *                 "<fn>: max_rounds = <r> is below 1",
 *                 "<fn>: alpha_q * eps_q = <product> is below 65536 (alpha_q = <a>, eps_q = <e>)";
 *               nothing is launched.
 * kernel_ms (may be NULL): HIP-event time of the sweep kernels and the table clears on the context's stream, summed over the
 * internal passes.  Temporary device buffers are freed on every exit path. */
int gg_ppr_topk(gg_ctx *ctx, const int32_t *rows /* [n_rows] */, int64_t n_rows, int32_t k, uint32_t alpha_q, uint64_t eps_q, int32_t max_rounds,
                int32_t exclude, int64_t scratch_bytes, int32_t *out_col /* [n_rows, k] */, uint64_t *out_score /* [n_rows, k] */,
                int32_t *n_pos /* [n_rows] */, int32_t *rounds /* [n_rows] */, int32_t *converged /* [n_rows] */, uint64_t *residual /* [n_rows] */,
                double *kernel_ms /* or NULL */);
int gg_ppr_rank(gg_ctx *ctx, const int32_t *u /* [m] */, const int32_t *v /* [m] */, int64_t m, uint32_t alpha_q, uint64_t eps_q, int32_t max_rounds,
                int32_t exclude, int64_t scratch_bytes, uint64_t *score /* [m] */, int32_t *ahead /* [m] */, int32_t *n_pos /* [m] */,
                int32_t *pos_below /* [m] */, int32_t *rounds /* [m] */, int32_t *converged /* [m] */, uint64_t *residual /* [m] */,
                double *kernel_ms /* or NULL */);

/* ---- spanning-forest sweep (additive entry points; GG_ABI_VERSION stays 9: no existing symbol, struct or behaviour changes).
 * The undirected edge list of the resident training graph, its minimum spanning forest under distinct integer keys and its
 * connected components -- what a train / test split needs to hold edges out without cutting the training graph apart
 * (graphgan_amd/split.py).  All on the set adjacency of the pair-neighbour sweep (sorted, distinct, no self-loop).  Needs
 * gg_set_graph_csr; no embedding table is read; every result is an integer.
 *
 * gg_undirected_edges: E = {(a, b) : a < b, b in N(a)} ordered by (a, b) ascending, j = 0 .. m - 1.  *m = |E|; edges int32 [m, 2]
 * is filled where it is not NULL (call once with NULL for m).  The list is built once per graph behind the set adjacency, kept on
 * the device and dropped by gg_set_graph_csr.
 *   limits      m not NULL ("gg_undirected_edges: m must not be NULL"); a resident graph ("gg_undirected_edges: needs the
 *               training graph (gg_set_graph_csr)"); "<fn>: the graph has <m> undirected edges, more than 2^31 - 1".
 *
 * gg_spanning_forest:
 *   key(j)      = (uint64(prio[j]) << 32) | j, prio the caller's uint32 [m] array (n_prio = m, its length); with prio NULL (n_prio
 *               is then not read) prio[j] = fmix32(j ^ fmix32(seed ^ 0x53504C54)), fmix32 the finaliser of the neighbour-mode
 *               sweep above.  Keys are distinct by construction, whatever the priorities.
 *   forest[j]   uint8 [m]: 1 exactly when Kruskal, taking the edges in ascending key order, takes edge j -- equivalently: no path
 *               between its ends uses only edges of smaller key.  This is the unique minimum spanning forest under the keys.
 *   component[v]  int32 [n_node]: the smallest node id of v's connected component; a node without an edge is its own component.
 *   stats       int64 [4] = {m, n_forest = the forest's edges, n_components = n_node - n_forest (isolated nodes count), rounds}.
 *   rounds      the Boruvka rounds that hooked at least one component.  A round: every current component takes its
 *               minimum-key edge to another component, and all of those edges are applied at once.
 *   forest and component may each be NULL (not computed / not copied).
 *   sweep_counts (int64 [GG_SF_MAX_SWEEPS, 2] or NULL): per edge sweep -- the rounds and the last one, which hooks nothing --
 *               (the edges between two components, the components hooked); -1 behind the last sweep.  sweep_ms (double
 *               [GG_SF_MAX_SWEEPS] or NULL): HIP-event time of each sweep with its pointer jumps; -1 behind the last.
 *   bit contract  integers only, and the forest is unique: the outputs are a function of the graph and the keys alone -- not of
 *               the grid, the order of the atomics or the run.
 *   shape       a round is two sweeps of one thread per edge.  sf_min: an edge between two components asks for the 64-bit
 *               unsigned minimum of its key on best[component] of both ends (vector global atomics); the asks of a wavefront's
 *               consecutive lanes for one component are folded into one, and an ask that a relaxed load shows cannot lower the
 *               word is dropped.  sf_hook: the edge whose key is best[c] sets forest[j] and parent[c] = the other component; two
 *               components that chose each other -- the only cycle distinct keys allow -- write parent[max] = min alone.  Each
 *               root is written by exactly one edge.  The hooks are counted per wavefront into one device word, the one word that
 *               crosses to the host per round.  Then parent <- parent[parent] in ceil(log2(components)) + 1 launches (a round may
 *               hook a chain as long as the graph) and comp[v] = parent[comp[v]].  At the end the smallest id per component by a
 *               32-bit integer minimum.  The loop ends at the first round that hooks nothing; nothing on the device loops on a
 *               condition.  State buffers live in the context and keep their capacity across calls.
 *   limits      stats not NULL ("gg_spanning_forest: stats must not be NULL"); "gg_spanning_forest: priority has <k> entries, the
 *               graph has <m> undirected edges"; "gg_spanning_forest: needs the training graph (gg_set_graph_csr)"; GG_EINVAL,
 *               nothing is launched.  More than ceil(log2(max(n_node, 2))) + 1 rounds cannot happen: GG_ECAPACITY,
 *               "gg_spanning_forest: internal error: more than <k> rounds on <n> nodes".
 * kernel_ms (may be NULL): HIP-event time of the whole forest on the context's stream, with its per-round read-backs. */
#define GG_SF_MAX_SWEEPS 34
int gg_undirected_edges(gg_ctx *ctx, int64_t *m, int32_t *edges /* [m, 2] or NULL */);
int gg_spanning_forest(gg_ctx *ctx, uint32_t seed, const uint32_t *prio /* [m] or NULL */, int64_t n_prio, uint8_t *forest /* [m] or NULL */,
                       int32_t *component /* [n_node] or NULL */, int64_t *stats /* [4] */, int64_t *sweep_counts /* [GG_SF_MAX_SWEEPS, 2] or NULL */,
                       double *sweep_ms /* [GG_SF_MAX_SWEEPS] or NULL */, double *kernel_ms /* or NULL */);

/* ---- pair consumer (additive entry point; GG_ABI_VERSION stays 9: no existing symbol, struct or behaviour changes).
 * gg_top_pairs: the k best-scored pairs of the WHOLE node set -- "which k pairs are the most likely missing edges" -- in one
 * sweep of the matrix-core tile stream (gg_all_score_reduce, gg_topk_scores, gg_rank_scores, gg_silhouette): nothing of size
 * rows x columns exists at any time.
 *   inputs      which (0 = generator, 1 = discriminator); precision 0 fp32 / 1 bf16 (n_emb <= 512); nodes: NULL = every node
 *               (m is not read), or m node ids, STRICTLY ascending (m may be 0); k in [1, 2^20]; exclude 0 / 1 (1 needs
 *               gg_set_graph_csr); buffer_entries: 0 = the default max(2^22, 4 k), else in [k + 4096, 2^26].
 *   candidates  the unordered pairs {u, v} of members of `nodes` with u < v, each once; with exclude = 1 without the pairs whose v
 *               is in u's list of the resident training graph (duplicates and self-loops in a list are fine).  (u, u) is never a
 *               candidate.
 *   score       s(u, v) = E[u] . E[v], fp32, NO bias, u (the smaller id) the ROW and v the COLUMN of the tile stream: the bits
 *               gg_rank_scores reports for (u, v) at that precision (precision 0: the k-ordered fmaf chain from 0.0 of gg_all_score;
 *               precision 1: v_mfma_f32_32x32x16_bf16 on the bf16 copy).
 *   order       (u, v) is ahead of (u', v') when ord(s) > ord(s'), or the ords are equal and (u, v) < (u', v') lexicographically;
 *               ord is that of gg_topk_scores' key, -0 counts as +0.
 *   results     u_out, v_out int32 [k], score_out fp32 [k]: the best pairs in that order; *n_found = min(k, candidates); the
 *               entries behind n_found are -1, -1, -inf.  m < 2 gives n_found = 0, not an error.
 *               stats (int64 [6] or NULL) = {launches, retries, compactions, appended entries, microseconds of host time in the
 *               compactions, the buffer's entries}.  ms (or NULL): HIP-event time of the whole sweep on the context's stream,
 *               with its read-backs and compactions (the bf16 copy excluded, as in gg_topk_scores).
 *   bit contract  u, v, score and n_found are a function of the table, the set and the graph alone -- not of buffer_entries, the
 *               grid, the order of the appends or the run.  Non-finite scores: unspecified.
 *   shape       One floor triple (fs, fu, fv) in device memory: the k-th best pair known, below everything until k are known;
 *               a kernel reads it once.  Per tile and lane 16 compares acc >= fs and one ballot; behind a hit the triple compare,
 *               column > row, the set's bit of the column, the binary search of the exclusion, and an append of (score bits, u, v)
 *               to a buffer with ONE integer atomic per wavefront on the fill counter -- it counts on past the capacity, the
 *               stores do not.  A launch is a rectangle of 32-row tiles x a column range in multiples of 128; a row tile starts at
 *               the 128-column tile of its smallest id.  One 4-byte read-back per launch; on overflow the counter is set back and
 *               the rectangle rerun as two halves (rows first, then columns); the first rectangle holds at most buffer_entries - k
 *               pairs, later ones double, up to 4 096 rows x all columns and 2^32 - 2^27 pairs (the counter has 32 bits).  A compaction
 *               (on the host: a selection among at most buffer_entries triples; when the fill passes min(k + (buffer_entries - k) / 2,
 *               max(3 k, 2^16)), and at the end, where the k best are sorted) keeps the k best and stores the k-th as the floor.
 *   limits      GG_EINVAL, nothing is launched, the text names gg_top_pairs: "which must be 0 (generator) or 1 (discriminator)",
 *               "precision must be 0 (fp32) or 1 (bf16)", "exclude must be 0 or 1", "k = <k> outside [1, 2^20]",
 *               "buffer_entries = <b> outside [k + 4096, 2^26] (0: the default)", "exclude = 1 needs the training graph
 *               (gg_set_graph_csr)", "bf16 supports n_emb <= 512 (got <d>)", "fp32 supports n_emb <= 1116 (got <d>)",
 *               "nodes[<i>] = <id> out of range [0, <n>)", "nodes[<i>] = <id> is not above nodes[<i - 1>] = <id> (strictly
 *               ascending ids)" (the FIRST bad index), "bad argument" (a NULL output). */
int gg_top_pairs(gg_ctx *ctx, int32_t which, int32_t precision, const int32_t *nodes /* [m] or NULL */, int64_t m, int64_t k, int32_t exclude,
                 int64_t buffer_entries, int32_t *u_out /* [k] */, int32_t *v_out /* [k] */, float *score_out /* [k] */, int64_t *n_found,
                 int64_t *stats /* [6] or NULL */, double *ms /* or NULL */);

/* sess.run(embedding_matrix) (graph_gan.py:298); which: 0 = generator, 1 = discriminator
 * (config.modes order, config.py:1).  out is [n_node, n_emb] fp32, unpadded. */
int gg_get_embeddings(gg_ctx *ctx, int32_t which, float *out);
int gg_get_bias(gg_ctx *ctx, int32_t which, float *out);
/* gg_write_embeddings: write_embeddings_to_file (graph_gan.py:293-306) for one model, byte-identical to
 * the reference's text (header "N\td\n"; rows "id\tv0\t...\n"; str(float64(fp32)) per value), formatted by
 * host threads.  gg_host_write_embeddings: the same for a caller-supplied [n_node, n_emb] fp32 matrix. */
int gg_write_embeddings(gg_ctx *ctx, int32_t which, const char *path, int32_t n_threads);
int gg_host_write_embeddings(const float *emb, int64_t n_node, int32_t n_emb, const char *path, int32_t n_threads);
/* gg_write_embeddings_bin: binary side-car of that text for large N: {"GGEB", version 1 i32, n_emb i32, n_node i64} + fp32 rows. */
int gg_write_embeddings_bin(gg_ctx *ctx, int32_t which, const char *path);
/* gg_edge_scores: the evaluator's scores (src/evaluation/link_prediction.py:26-27: np.dot(emd[u], emd[v]) per test /
 * negative edge) computed on the device from the resident table of model `which`, in float64 like the reference. */
int gg_edge_scores(gg_ctx *ctx, int32_t which, const int32_t *u, const int32_t *v, int64_t n, double *out);
int gg_set_embeddings(gg_ctx *ctx, int32_t which, const float *emb);
int gg_set_bias(gg_ctx *ctx, int32_t which, const float *bias);

/* tf.train.Saver save/restore (graph_gan.py:55,124-127,137-138): all variables + Adam
 * slots + step counts, as one flat binary file (format: DESIGN.md). */
int gg_save_state(gg_ctx *ctx, const char *path);
int gg_load_state(gg_ctx *ctx, const char *path);

int gg_get_counters(gg_ctx *ctx, gg_counters *out);

/* Profiling cadence.  every_n = 1 (default): HIP events bracket every walk launch, every level_score_kernel launch
 * and every gg_*_pass, and the passes wait for theirs (synchronous, last_kernel_ms valid).  every_n = k > 1: only
 * every k-th walk launch carries events (an event pair costs ~6 us of stream bubble on each side, ~0.1 ms per walk
 * call), and gg_d_pass / gg_g_pass return as soon as their kernels are enqueued -- stream-ordered before whatever
 * is called next; the next call that returns data, gg_synchronize or gg_comm_barrier waits for them and reports
 * their errors.  every_n = 0: no events at all.  Also settable as GG_PROFILE_EVERY. */
int gg_set_profiling(gg_ctx *ctx, int32_t every_n);
/* gg_set_profiling_solo: solo = 1 (default): a profiled side-stream walk first waits for the main stream, so its kernels
 * are measured ALONE; solo = 0: it runs beside the discriminator update like every other launch (overlapped figure). */
int gg_set_profiling_solo(gg_ctx *ctx, int32_t solo);
/* Wait for everything enqueued on the context's stream. */
int gg_synchronize(gg_ctx *ctx);

/* ---- multi-GPU (no reference counterpart: single tf.Session, graph_gan.py:57-61).
 * One process per GPU.  Rank 0 calls gg_comm_unique_id, the 128 bytes travel by any side
 * channel, every rank calls gg_comm_init.  Afterwards each optimizer step sums the
 * gradients of all ranks (RCCL all-reduce on the context's stream) before the update,
 * so replicas stay identical. */
int gg_comm_unique_id(void *id128);
int gg_comm_init(gg_ctx *ctx, const void *id128, int32_t rank, int32_t world);
int gg_comm_barrier(gg_ctx *ctx);
/* gg_comm_stats: out4 = {optimizer steps that exchanged row packs (sparse), steps that exchanged the whole accumulators
 * (dense: reduce-scatter + all-gather), bytes this rank has sent for gradient exchanges so far, world size}. */
int gg_comm_stats(gg_ctx *ctx, int64_t *out4);
/* gg_comm_stats_ex (ABI 6): out8 = {steps that all-gathered fixed-capacity row packs, steps that took the owner-partitioned
 * exchange (send / recv to the rows' owners + all-gather of the reduced rows), dense steps, bytes sent, world size,
 * 1 if the owner-partitioned exchange moves bf16 rows (GG_COMM_BF16=1), 0, 0}.  The first two add up to out4[0]. */
int gg_comm_stats_ex(gg_ctx *ctx, int64_t *out8);

/* ---- edge-list ingest: utils.read_edges (utils.py:12-54) natively -- adjacency CSR in the reference's
 * list order from the train file (+ node ids of the test file); buffers are malloc'ed by the library and
 * released with gg_host_free_graph.  No GPU, no ctx. */
typedef struct gg_graph {
    int32_t n_node;
    int64_t nnz;            /* = 2 * n_train_edges */
    int64_t n_train_edges, n_test_edges;
    int64_t *rowptr;        /* [n_node + 1] */
    int32_t *col;           /* [nnz] */
} gg_graph;
int gg_host_read_edges(const char *train_path, const char *test_path /* may be NULL or "" */, gg_graph *out);
void gg_host_free_graph(gg_graph *g);

/* ---- synthetic power-law graphs for the benchmark configs (BASELINE.json configs[2..4];
 * recipe in SURVEY.md section 8d): Barabasi-Albert, m edges per new node, node ids permuted.
 * edges_out: [n_edges_cap][2] int32; returns the number of edges written or GG_E*. */
int64_t gg_synth_powerlaw(int32_t n_node, int32_t m, uint64_t seed_graph, uint64_t seed_perm,
                          int32_t *edges_out, int64_t n_edges_cap);

#ifdef __cplusplus
}
#endif
#endif /* GRAPHGAN_HIP_H */
