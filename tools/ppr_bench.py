#!/usr/bin/env python3
"""The push sweep (gg_ppr_topk / gg_ppr_rank: rooted PageRank by local push) on the synthetic power-law workload, 10^6 nodes / 10^7
edges, with the default parameters (alpha 0.15, eps 1e-4, 200 rounds), beside the two-hop sweep with "aa" on the same queries in
the same run.
    python tools/ppr_bench.py [n_node] [out.json]        (default 10^6 profiles/r28_ppr_bench.json)
One JSON line, printed and written to the output file.  HIP events, three alternating runs of the legs in one process, the best
of the three:
    ppr_topk        the top-100 lists of 4 096 random query nodes;
    ppr_rank        the ranks of 65 536 random training-edge pairs (u, v) sorted by u, so that a root is pushed once (device time;
                    the host derivation of the full rank is outside);
    two_hop_topk    Engine.two_hop_topk(k=100, weights=aa) on the same nodes;
    two_hop_rank    Engine.two_hop_rank(weights=aa) on the same pairs.
Reported beside them: pushed adjacency entries per second (the sum of deg over all pushes / device time; the numerator comes from
the numpy rounds on the host, exactly for the random-node leg -- whose outputs are also compared bit for bit with the device's --
and from a sample of 1 024 roots for the rank leg), the mean and the largest `rounds`, the share of queries with global tables,
the bytes of table scratch and the number of passes.
EXPECTATION, written before the first run: pushed entries per second on the random-node leg >= the two-hop sweep's expansion
rate (sum of T / device time) on the same random nodes in the same run.  A push round moves the same kind of entry through the same
table as the two-hop fill, but it pays two barriers per round, a 64-bit division per push, the degree lookup of every target and
zeroed global tables sized for the bound, not for the use; r25 recorded 2.7e9 expansion entries/s for the two-hop sweep on random
nodes and nobody has measured the push.  "expectation" reports HELD or NOT with the ratio.  It is a finding, not a gate.
What is NOT measured: a kernel trace; counters; any table size, hash, group width, scratch cap or grid other than the first; other
parameters than the defaults; real datasets at this size."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import graphgan_amd as ga  # noqa: E402
from graphgan_amd import workloads  # noqa: E402
from graphgan_amd.evaluation import graph_ppr as gp  # noqa: E402
from graphgan_amd.evaluation import graph_ranking as gr  # noqa: E402
from graphgan_amd.evaluation import link_heuristics as lh  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
dest = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r28_ppr_bench.json")
N_TOPK, N_RANK, K, N_SAMPLE = 4096, 65536, 100, 1024
ALPHA, EPS, MAX_ROUNDS = gp.DEFAULT_ALPHA, gp.DEFAULT_EPS, gp.DEFAULT_MAX_ROUNDS

t0 = time.time()
rowptr, col, emb, n_edges = workloads.powerlaw_workload(n, n_emb=4)  # (the sweeps read no embedding; a context needs tables)
t_gen = time.time() - t0
eng = ga.Engine(emb, emb, optimizer=ga.GG_OPT_SGD)
eng.set_graph_csr(rowptr, col)
deg = eng.distinct_degrees().astype(np.int64)
ptr, adj = lh.csr_set_adjacency(rowptr, col)
src = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
T_node = np.bincount(src, weights=deg[adj].astype(np.float64), minlength=n).astype(np.int64)  # the two-hop expansion of every node

rs = np.random.default_rng(5)
rows = rs.integers(0, n, N_TOPK).astype(np.int32)
at = np.sort(rs.integers(0, len(adj), N_RANK))  # random entries of the adjacency = random training edges; ascending = sorted by u
u, v = src[at].astype(np.int32), adj[at].astype(np.int32)
roots_r = np.unique(u)
w_aa = gr.index_weights("aa", deg)

alpha_q, eps_q = gp.quantise(ALPHA, EPS)
E = gp.touched_bound(n, alpha_q, eps_q)
slots = 256
while slots < 2 * E:
    slots *= 2
is_global = E > ga.Engine.PPR_LDS_CAP
fcap = (E + 1) // 2 * 2
task_bytes = 8 * (2 * slots + slots // 2 + fcap + 3 * (fcap // 2)) if is_global else 0
SCRATCH = 2048 << 20  # the default cap of gg_ppr_*
per_pass = max(1, SCRATCH // task_bytes) if is_global else 0


def tables(n_task):
    return {"global_share": float(is_global), "table_slots": slots, "task_bytes": task_bytes, "tasks": int(n_task),
            "scratch_bytes_per_pass": int(min(per_pass, n_task) * task_bytes), "passes": int(-(-n_task // per_pass)) if is_global else 1}


out = {"workload": "push sweep: power-law graph of %d nodes / %d edges (%d adjacency entries); alpha=%s eps=%s max_rounds=%d (alpha_q=%d eps_q=%d); top-%d of %d "
                   "random nodes, ranks of %d random training-edge pairs sorted by u (%d distinct roots)"
                   % (n, n_edges, len(adj), ALPHA, EPS, MAX_ROUNDS, alpha_q, eps_q, K, N_TOPK, N_RANK, len(roots_r)),
       "workload_gen_s": t_gen, "max_distinct_degree": int(deg.max()), "mean_distinct_degree": float(deg.mean()), "lds_cap": ga.Engine.PPR_LDS_CAP,
       "touched_bound_E": int(E), "topk_tables": tables(N_TOPK), "rank_tables": tables(len(roots_r)),
       "expectation_text": "pushed adjacency entries per second of ppr_topk on the random nodes >= expansion entries per second of two_hop_topk (aa) on the same "
                           "nodes in the same run",
       "not_measured": ["a kernel trace", "counters", "any table size, hash, group width, scratch cap or grid other than the first",
                        "other parameters than the defaults", "real datasets at this size"]}

kw = dict(alpha=ALPHA, eps=EPS, max_rounds=MAX_ROUNDS)
eng.ppr_rank(u[:64], v[:64], **kw)  # (builds the host neighbour sets of the rank derivation; not timed)
best = {}


def leg(name, ms):
    best[name] = min(best.get(name, 1e30), ms)


for _ in range(3):  # alternating, so that every leg sees the same clocks
    leg("ppr_topk", eng.ppr_topk(rows, k=K, **kw)["ms"])
    leg("two_hop_topk_aa", eng.two_hop_topk(rows, k=K, weights=w_aa)["ms"])
    leg("ppr_rank", eng.ppr_rank(u, v, **kw)["ms"])
    leg("two_hop_rank_aa", eng.two_hop_rank(u, v, weights=w_aa)["ms"])
res_t, res_r = eng.ppr_topk(rows, k=K, **kw), eng.ppr_rank(u, v, **kw)
th_r = eng.two_hop_rank(u, v, weights=w_aa)
eng.close()
print("device legs done: %s; the host rounds follow" % json.dumps(best), file=sys.stderr, flush=True)

# the numerators, from the numpy rounds on the host
t0 = time.time()
host_t = gp.host_ppr_topk(ptr, adj, rows, K, ALPHA, EPS, MAX_ROUNDS, True)
t_host = time.time() - t0
bits = all(np.array_equal(res_t[key], host_t[key]) for key in ("col", "score", "n_pos", "rounds", "converged", "residual"))
sample = roots_r[rs.permutation(len(roots_r))[:N_SAMPLE]]
pushed_sample = gp.host_ppr_topk(ptr, adj, sample, 1, ALPHA, EPS, MAX_ROUNDS, True)["pushed"]
pushed_t = int(host_t["pushed"].sum())
pushed_r = float(pushed_sample.mean()) * len(roots_r)

out["ms"] = best
out["queries_per_s"] = {"ppr_topk": N_TOPK / (best["ppr_topk"] * 1e-3), "ppr_rank": N_RANK / (best["ppr_rank"] * 1e-3)}
out["pushed_entries"] = {"ppr_topk": pushed_t, "ppr_topk_mean_per_query": pushed_t / N_TOPK, "ppr_rank_estimate_from_%d_roots" % len(sample): pushed_r,
                         "bound_B_per_query": int((1 << 40) // ((eps_q * alpha_q) >> 16))}
out["pushed_entries_per_s"] = {"ppr_topk": pushed_t / (best["ppr_topk"] * 1e-3), "ppr_rank_estimate": pushed_r / (best["ppr_rank"] * 1e-3)}
out["two_hop_expansion_entries_per_s"] = {"two_hop_topk_aa": float(T_node[rows].sum()) / (best["two_hop_topk_aa"] * 1e-3),
                                          "two_hop_rank_aa": float(T_node[u].sum()) / (best["two_hop_rank_aa"] * 1e-3)}
out["rounds"] = {"topk_mean": float(res_t["rounds"].mean()), "topk_largest": int(res_t["rounds"].max()), "rank_mean": float(res_r["rounds"].mean()),
                 "rank_largest": int(res_r["rounds"].max()), "converged_share": float(res_t["converged"].mean()),
                 "mean_residual": float(res_t["residual"].astype(np.float64).mean() / 2.0 ** 40)}
out["results"] = {"device_bits_equal_host_on_the_random_nodes": bool(bits), "host_numpy_s_for_the_random_nodes": t_host,
                  "topk_full_lists_share": float((res_t["n_pos"] >= K).mean()), "rank_reach": float((res_r["score"] > 0).mean()),
                  "rank_mrr_unfiltered": float(np.mean(1.0 / res_r["rank"])), "two_hop_aa_rank_reach": float((th_r["score"] > 0).mean()),
                  "two_hop_aa_rank_mrr_unfiltered": float(np.mean(1.0 / th_r["rank"]))}
ratio = out["pushed_entries_per_s"]["ppr_topk"] / out["two_hop_expansion_entries_per_s"]["two_hop_topk_aa"]
out["ppr_over_two_hop_entry_rate"] = ratio
out["expectation"] = "%s (%.3f x the two-hop sweep's expansion rate on the same random nodes)" % ("HELD" if ratio >= 1.0 else "NOT", ratio)
line = json.dumps(out)
os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
with open(dest, "w") as f:
    f.write(line + "\n")
print(line)
