#!/usr/bin/env python3
"""The two-hop sweep (gg_two_hop_topk / gg_two_hop_rank) on the synthetic power-law workload, 10^6 nodes / 10^7 edges, beside the
embedding side of the same question on the same queries in the same run.
    python tools/two_hop_bench.py [n_node] [n_emb] [out.json]        (default 10^6 128 profiles/r25_two_hop_bench.json)
One JSON line, printed and written to the output file.  HIP events, three alternating runs of the legs in one process, the best
of the three:
    two_hop_topk    the top-100 lists of 4 096 random query nodes, for "cn" (no weights) and "aa" (fixed-point Adamic-Adar weights);
    two_hop_rank    the ranks of 65 536 random training-edge pairs (u, v), for "cn" and "aa" (device time; the host derivation of the
                    full rank is outside);
    emb_topk        Engine.topk(k=100, precision="bf16", exclude=True) on the same query nodes;
    emb_rank        Engine.rank(..., precision="bf16", exclude=True) on the same pairs.
Reported beside them: the share of queries per table class (LDS up to Engine.TWO_HOP_LDS_CAP expansion entries, global above), the
largest and the mean expansion T, the passes the default scratch cap makes of the global-table queries, and the host time of the
neighbour sets the rank derivation needs.
EXPECTATION, written before the first run: the graph side of the question costs no more than the embedding side -- two_hop_topk
(either index) <= emb_topk and two_hop_rank (either index) <= emb_rank.  A query touches T entries of the adjacency where the
embedding side streams the whole table per block of rows, but the training-edge queries of this graph are hub-heavy and run one
workgroup each on tables in global memory; nobody has measured either leg on these queries.  "expectation" reports HELD or NOT per
leg with the ratios.  It is a finding, not a gate.
What is NOT measured: a kernel trace; counters; any table size, hash, group width, scratch cap or grid other than the first; the
radix select against a full sort; real datasets at this size."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import graphgan_amd as ga  # noqa: E402
from graphgan_amd import workloads  # noqa: E402
from graphgan_amd.evaluation import graph_ranking as gr  # noqa: E402
from graphgan_amd.evaluation import link_heuristics as lh  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 128
dest = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r25_two_hop_bench.json")
N_TOPK, N_RANK, K = 4096, 65536, 100

t0 = time.time()
rowptr, col, emb, n_edges = workloads.powerlaw_workload(n, n_emb=d)
t_gen = time.time() - t0
eng = ga.Engine(emb, emb, optimizer=ga.GG_OPT_SGD)  # SGD: no Adam slots
eng.set_graph_csr(rowptr, col)
deg = eng.distinct_degrees().astype(np.int64)  # (builds the set adjacency: host sort + upload, once per graph)
t0 = time.time()
ptr, adj = lh.csr_set_adjacency(rowptr, col)
t_sets = time.time() - t0
src = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
T_node = np.bincount(src, weights=deg[adj].astype(np.float64), minlength=n).astype(np.int64)  # (exact: far below 2^53)

rs = np.random.default_rng(5)
rows = rs.integers(0, n, N_TOPK).astype(np.int32)
at = rs.integers(0, len(adj), N_RANK)  # a random entry of the adjacency = a random training edge in a random direction
u, v = src[at].astype(np.int32), adj[at].astype(np.int32)
cap = ga.Engine.TWO_HOP_LDS_CAP
w_aa = gr.index_weights("aa", deg)


def classes(q):
    T = T_node[q]
    slots = np.maximum(256, 2 ** np.ceil(np.log2(np.maximum(2 * np.minimum(T, n), 1))).astype(np.int64))
    glob = T > cap
    return {"lds_share": float((~glob).mean()), "global_share": float(glob.mean()), "largest_T": int(T.max()), "mean_T": float(T.mean()),
            "global_table_bytes": int((slots[glob] * 12).sum()), "passes_at_default_scratch": int(np.ceil((slots[glob] * 12).sum() / (256 << 20)))}


out = {"workload": "two-hop sweep: power-law graph of %d nodes / %d edges (%d adjacency entries), n_emb=%d; top-%d of %d random nodes, ranks of %d random "
                   "training-edge pairs" % (n, n_edges, len(adj), d, K, N_TOPK, N_RANK),
       "workload_gen_s": t_gen, "host_neighbour_sets_s": t_sets, "max_distinct_degree": int(deg.max()), "mean_distinct_degree": float(deg.mean()), "lds_cap": cap,
       "topk_queries": classes(rows), "rank_queries": classes(u),
       "expectation_text": "two_hop_topk (cn, aa) <= Engine.topk bf16 exclude and two_hop_rank (cn, aa) <= Engine.rank bf16 exclude on the same queries",
       "not_measured": ["a kernel trace", "counters", "any table size, hash, group width, scratch cap or grid other than the first",
                        "the radix select against a full sort", "real datasets at this size"]}

eng.two_hop_rank(u[:64], v[:64])  # (builds the host neighbour sets of the rank derivation; not timed)
best = {}


def leg(name, ms):
    best[name] = min(best.get(name, 1e30), ms)


for _ in range(3):  # alternating, so that every leg sees the same clocks
    leg("two_hop_topk_cn", eng.two_hop_topk(rows, k=K)["ms"])
    leg("two_hop_topk_aa", eng.two_hop_topk(rows, k=K, weights=w_aa)["ms"])
    leg("emb_topk", eng.topk(rows, k=K, precision="bf16", exclude=True)["kernel_ms"])
    leg("two_hop_rank_cn", eng.two_hop_rank(u, v)["ms"])
    leg("two_hop_rank_aa", eng.two_hop_rank(u, v, weights=w_aa)["ms"])
    leg("emb_rank", eng.rank(u, v, precision="bf16", exclude=True)["kernel_ms"])
res_t, res_r = eng.two_hop_topk(rows, k=K, weights=w_aa), eng.two_hop_rank(u, v, weights=w_aa)
eng.close()

out["ms"] = best
out["queries_per_s"] = {"two_hop_topk_aa": N_TOPK / (best["two_hop_topk_aa"] * 1e-3), "two_hop_rank_aa": N_RANK / (best["two_hop_rank_aa"] * 1e-3)}
out["expansion_entries_per_s"] = {"two_hop_topk_aa": float(T_node[rows].sum()) / (best["two_hop_topk_aa"] * 1e-3),
                                  "two_hop_rank_aa": float(T_node[u].sum()) / (best["two_hop_rank_aa"] * 1e-3)}
out["results"] = {"topk_full_lists_share": float((res_t["n_pos"] >= K).mean()), "rank_reach": float((res_r["score"] > 0).mean()),
                  "rank_mrr_unfiltered": float(np.mean(1.0 / res_r["rank"]))}
ratio_t = max(best["two_hop_topk_cn"], best["two_hop_topk_aa"]) / best["emb_topk"]
ratio_r = max(best["two_hop_rank_cn"], best["two_hop_rank_aa"]) / best["emb_rank"]
out["two_hop_over_emb"] = {"topk": ratio_t, "rank": ratio_r}
out["expectation"] = "top-K %s (%.2f x the embedding side), rank %s (%.2f x)" % ("HELD" if ratio_t <= 1.0 else "NOT", ratio_t, "HELD" if ratio_r <= 1.0 else "NOT", ratio_r)
line = json.dumps(out)
os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
with open(dest, "w") as f:
    f.write(line + "\n")
print(line)
