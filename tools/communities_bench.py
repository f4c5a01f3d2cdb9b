#!/usr/bin/env python3
"""Label propagation (gg_label_propagation), its neighbour-mode sweep (gg_neighbor_mode) and the partition edge counts
(gg_partition_edges) on the synthetic power-law workload: 10^6 nodes / 10^7 edges.
    python tools/communities_bench.py [n_node] [iters] [out.json]        (default 10^6 8 profiles/r24_communities_bench.json)
One JSON line, printed and written to the output file.  HIP events, three alternating runs of the legs in one process, the best
of the three:
    lpa             gg_label_propagation capped at `iters` iterations, reported as ms per iteration (both half-steps and the
                    4-byte read-back between iterations);
    neighbor_mode   one gg_neighbor_mode over all nodes on the labels the fit ended with (kernel time; the upload is outside);
    partition_edges one gg_partition_edges on the communities the fit ended with;
    neighbor_sum    one gg_neighbor_sum at n_col = 8 over all nodes in the same run, the yardstick.
The share of nodes and of adjacency entries per path (lane groups of 4 / 16 / 64, the LDS table, the global table) comes from the
distinct degrees; the single-thread host rate (numpy, evaluation/graph_communities.py) from one neighbour-mode call on a
sample graph of n / 20 nodes.
EXPECTATION, written before the first run: an iteration gathers one 4-byte label per adjacency entry where the neighbour-sum
sweep at n_col = 8 gathers a 32-byte row, so an iteration should cost no more than that sweep; "expectation" reports HELD or NOT
with the ratio.  It is a finding, not a gate.
Byte model per iteration: entries x (4 B id + 4 B label) + 2 x 4 B per node (the label read and written), as a fraction of the
6.29 TB/s float4 copy rate.
What is NOT measured: a kernel trace; counters; any group width, table size, hash, chunk length or grid other than the first;
NMI on any labelled real dataset."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import graphgan_amd as ga  # noqa: E402
from graphgan_amd.evaluation import graph_communities as gcomm  # noqa: E402
from graphgan_amd.evaluation import link_heuristics as lh  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
T = int(sys.argv[2]) if len(sys.argv) > 2 else 8
dest = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r24_communities_bench.json")
COPY_TBPS = 6.29

t0 = time.time()
edges = ga.synth_powerlaw(n, 10, 1, 2)
rowptr, col = ga.edges_to_csr(n, edges)
t_gen = time.time() - t0
table = np.zeros((n, 4), np.float32)  # (the sweeps read no embedding; a context needs tables)
eng = ga.Engine(table, table, optimizer=ga.GG_OPT_SGD)
eng.set_graph_csr(rowptr, col)
t0 = time.time()
deg = eng.distinct_degrees().astype(np.int64)  # (builds the set adjacency: host sort + upload, once per graph)
t_adj = time.time() - t0
entries = int(deg.sum())
cap = ga.Engine.NEIGHBOR_MODE_LDS_CAP
paths = {"group4": deg <= 4, "group16": (deg > 4) & (deg <= 16), "group64": (deg > 16) & (deg <= 64), "lds_table": (deg > 64) & (deg <= cap),
         "global_table": deg > cap}
model = entries * 8.0 + 2.0 * 4.0 * n

out = {"workload": "label propagation: power-law graph of %d nodes / %d edges (%d adjacency entries), at most %d iterations, seed 0" % (n, len(edges), entries, T),
       "workload_gen_s": t_gen, "set_adjacency_s": t_adj, "max_distinct_degree": int(deg.max()), "mean_distinct_degree": float(deg.mean()),
       "lds_cap": cap,
       "paths": {k: {"nodes": int(m.sum()), "node_share": float(m.mean()), "entry_share": float(deg[m].sum() / entries)} for k, m in paths.items()},
       "expectation_text": "an LPA iteration (both half-steps) costs no more than one gg_neighbor_sum at n_col = 8 in the same run",
       "model_bytes_per_iteration": model,
       "not_measured": ["a kernel trace", "counters", "any group width, table size, hash, chunk length or grid other than the first",
                        "NMI on any labelled real dataset"]}

X = np.random.default_rng(12).standard_normal((n, 8), dtype=np.float32)
fit = eng.label_propagation(seed=0, max_iters=T)  # (builds the plans; not timed)
comm, k = gcomm.relabel(fit["labels"])
best = {}
for _ in range(3):  # alternating, so that every leg sees the same clocks
    fit = eng.label_propagation(seed=0, max_iters=T)
    best["lpa"] = min(best.get("lpa", 1e30), fit["ms"] / fit["iters"])
    best["mode"] = min(best.get("mode", 1e30), eng.neighbor_mode(fit["labels"], salt=1)["ms"])
    cnt = eng.partition_edges(comm, k)
    best["edges"] = min(best.get("edges", 1e30), cnt["ms"])
    best["ns8"] = min(best.get("ns8", 1e30), eng.neighbor_sum(X)["ms"])
eng.close()


def leg(ms, bytes_):
    return {"ms": ms, "model_TBps": bytes_ / (ms * 1e-3) / 1e12, "of_copy_rate": bytes_ / (ms * 1e-3) / 1e12 / COPY_TBPS,
            "adjacency_entries_per_s": entries / (ms * 1e-3)}


out["lpa"] = dict(leg(best["lpa"], model), ms_per_iteration=best["lpa"], iters=fit["iters"], converged=fit["converged"], changed=fit["changed"].tolist(),
                  communities=k, modularity=gcomm.modularity_from_counts(cnt["intra"], cnt["tot"]))
out["neighbor_mode"] = leg(best["mode"], entries * 8.0 + 2.0 * 4.0 * n)
out["partition_edges"] = dict(leg(best["edges"], entries * 8.0 + 4.0 * n), n_label=k)
out["neighbor_sum_n_col_8"] = {"ms": best["ns8"]}
ratio = best["lpa"] / best["ns8"]
out["expectation"] = "%s: an iteration takes %.3f ms, %.2f x the neighbour-sum sweep's %.3f ms" % ("HELD" if ratio <= 1.0 else "NOT", best["lpa"], ratio, best["ns8"])
out["lpa_over_neighbor_sum"] = ratio

# the single-thread host rate on a sample graph
ns = max(1000, n // 20)
e_s = ga.synth_powerlaw(ns, 10, 1, 2)
ptr_s, adj_s = lh.set_adjacency(e_s, ns)
labels_s = np.random.default_rng(3).integers(0, ns, ns)
t0 = time.time()
gcomm.host_neighbor_mode(ptr_s, adj_s, labels_s, salt=1)
t_host = time.time() - t0
out["host_sample"] = {"nodes": ns, "entries": int(len(adj_s)), "neighbor_mode_s": t_host, "adjacency_entries_per_s": len(adj_s) / t_host,
                      "device_over_host_rate": (entries / (best["mode"] * 1e-3)) / (len(adj_s) / t_host)}
line = json.dumps(out)
os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
with open(dest, "w") as f:
    f.write(line + "\n")
print(line)
