#!/usr/bin/env python
"""The two-hop pair sweep (gg_two_hop_top_pairs) on the synthetic power-law workload, 10^6 nodes / 10^7 edges, beside the embedding
side of the same question, Engine.top_pairs(k, "bf16"), on the same graph in the same run.
    python tools/two_hop_pairs_bench.py [n_node] [n_emb] [k] [--out PATH]        (default 10^6 128 100000 profiles/r30_two_hop_pairs_bench.json)
One JSON line, also written to PATH.  Legs, all with exclude on and over all n nodes:
    two_hop_top_pairs_cn   the k best pairs by common neighbours;
    two_hop_top_pairs_aa   the k best pairs by the fixed-point Adamic-Adar weights;
    top_pairs_bf16         the k best pairs by E[u] . E[v], bf16 inputs (the r29 leg).
The legs ALTERNATE, three runs each, best of 3 (all runs are reported); ms are HIP-event times of the whole sweep with its
read-backs, table clears and host compactions; "stats" are those of every call, in the order of the runs; "call_s" is the wall time
of each leg's last call, with the host plan.
EXPECTATION, written before the first run and recorded as held or not, never gated: the graph side of the question costs no more
than the embedding side -- two_hop_top_pairs (cn and aa) <= top_pairs bf16 of this run.  Nobody has measured this sweep.  It visits
sum over w of deg(w)^2 / 2 expansion entries where the tile stream visits n^2 / 2 pairs at matrix-core rate, most of its sources
accumulate in zeroed tables in global memory, one workgroup per source, and the first batches run before any floor exists; the skip
bound B(u) < fs is the one thing on its side.  On a hub-heavy graph the expectation may well fail, as the two_hop_rank leg's did (r25).
What is NOT measured or tuned: a kernel trace; counters; the first batch (256 sources), the doubling, the largest batch, the
compaction threshold, the buffer size, the scratch cap, the table size, the hash, the 16-lane / workgroup split, the grid; a hub
source split over several workgroups; a compaction on the device; the share of the host plan and of the host compactions; real
datasets at this size."""
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

argv = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "r30_two_hop_pairs_bench.json")
if "--out" in argv:
    i = argv.index("--out")
    out_path = argv[i + 1]
    del argv[i:i + 2]
n = int(argv[0]) if len(argv) > 0 else 1_000_000
d = int(argv[1]) if len(argv) > 1 else 128
k = int(argv[2]) if len(argv) > 2 else 100_000

t0 = time.time()
rowptr, col, emb, n_edges = workloads.powerlaw_workload(n, n_emb=d)
t_gen = time.time() - t0
eng = ga.Engine(emb, emb, optimizer=ga.GG_OPT_SGD)  # SGD: no Adam slots
eng.set_graph_csr(rowptr, col)
deg = eng.distinct_degrees().astype(np.int64)  # (builds the set adjacency: host sort + upload, once per graph)
w_aa = gr.index_weights("aa", deg)

out = {"workload": "two-hop pair sweep: power-law graph of %d nodes / %d edges, all pairs, k=%d, exclude on; top_pairs bf16 at n_emb=%d on the same graph"
                   % (n, n_edges, k, d),
       "workload_gen_s": t_gen, "max_distinct_degree": int(deg.max()), "mean_distinct_degree": float(deg.mean()),
       "expansion_entries_upper_bound": float((deg.astype(np.float64) ** 2).sum() / 2), "pairs": n * (n - 1) // 2,
       "expectation_text": "two_hop_top_pairs (cn, aa) <= Engine.top_pairs bf16 on the same graph in the same run",
       "not_tuned": ["first batch", "batch doubling", "largest batch", "compaction threshold", "buffer size", "scratch cap", "table size", "hash",
                     "16-lane / workgroup split", "grid", "hub source over several workgroups", "device compaction"],
       "not_measured": ["a kernel trace", "counters", "the share of the host plan and the host compactions", "real datasets at this size"]}

small = np.arange(0, n, max(1, n // 4096)).astype(np.int32)
eng.two_hop_top_pairs(min(k, 1000), nodes=small)  # warm-up: a sample of the nodes
eng.top_pairs(min(k, 1000), nodes=small, precision="bf16")
runs = {"two_hop_top_pairs_cn": [], "two_hop_top_pairs_aa": [], "top_pairs_bf16": []}
stats = {name: [] for name in runs}
last, wall = {}, {}
for _ in range(3):  # alternating, so that every leg sees the same clocks
    for name, call in (("two_hop_top_pairs_cn", lambda: eng.two_hop_top_pairs(k, exclude=True)),
                       ("two_hop_top_pairs_aa", lambda: eng.two_hop_top_pairs(k, weights=w_aa, exclude=True)),
                       ("top_pairs_bf16", lambda: eng.top_pairs(k, precision="bf16", exclude=True))):
        t0 = time.time()
        res = call()
        wall[name] = time.time() - t0
        runs[name].append(res["ms"])
        stats[name].append(res["stats"])
        last[name] = res
eng.close()

best = {name: min(v) for name, v in runs.items()}
out["ms"] = best
out["runs_ms"] = runs
out["call_s"] = wall
out["stats"] = stats
out["results"] = {name: {"n_found": last[name]["n_found"], "first_score": float(last[name]["score"][0]), "kth_score": float(last[name]["score"][last[name]["n_found"] - 1])}
                  for name in runs}
ratio = max(best["two_hop_top_pairs_cn"], best["two_hop_top_pairs_aa"]) / best["top_pairs_bf16"]
out["two_hop_over_emb"] = {"cn": best["two_hop_top_pairs_cn"] / best["top_pairs_bf16"], "aa": best["two_hop_top_pairs_aa"] / best["top_pairs_bf16"]}
out["expectation"] = "%s (the slower index takes %.2f x the embedding side)" % ("HELD" if ratio <= 1.0 else "NOT", ratio)
line = json.dumps(out)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
print(line)
