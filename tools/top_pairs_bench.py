#!/usr/bin/env python3
"""Global top-K pair prediction (gg_top_pairs) on the synthetic power-law workload, beside the rank consumer of the same tile
stream (gg_rank_scores) in the SAME run:
    top_pairs   all n nodes, k = 10^5, exclude on: n (n - 1) / 2 pairs                 (n = 10^6: 5.0 10^11)
    rank        65 536 random queries over the n columns, exclude on: 65 536 n scores  (n = 10^6: 6.6 10^10)
    python tools/top_pairs_bench.py [n_node] [n_emb] [k] [queries] [--out PATH]        (default 10^6 128 100000 65536)
One JSON line, also written to PATH (default profiles/r29_top_pairs_bench.json).  Both precisions; the legs ALTERNATE, three runs
each, best of 3 (all runs are reported); ms are HIP-event times: top_pairs' cover the whole sweep with its per-launch read-backs
and its host compactions (whose share is reported from the call's stats), the rank's its gather and stream kernels.

EXPECTATION, written before the first run and recorded as held or not, never gated: time per pair of top_pairs <= 1.5 x time per
score of Engine.rank in the same run, per precision.  In the steady state the floor consumer costs the rank consumer's 16 compares
and one ballot per tile; what comes on top is the first rectangles (every pair is appended until k are known), the compactions
on the host and one read-back per launch.

Parity: the pairs top_pairs returns in fp32, sampled, carry the score bits Engine.rank(u, v, exclude=False) reports for them, none
of them is a training edge, and the list is in order."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

argv = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "r29_top_pairs_bench.json")
if "--out" in argv:
    i = argv.index("--out")
    out_path = argv[i + 1]
    del argv[i:i + 2]
n = int(argv[0]) if len(argv) > 0 else 1_000_000
d = int(argv[1]) if len(argv) > 1 else 128
k = int(argv[2]) if len(argv) > 2 else 100_000
nq = int(argv[3]) if len(argv) > 3 else 65536
RUNS = 3
EXPECTED_RATIO = 1.5

import graphgan_amd as ga  # noqa: E402
from graphgan_amd import workloads  # noqa: E402

t0 = time.time()
rowptr, col, emb, n_edges = workloads.powerlaw_workload(n, n_emb=d)
t_gen = time.time() - t0
eng = ga.Engine(emb, emb, optimizer=ga.GG_OPT_SGD)  # SGD: no Adam slots
eng.set_graph_csr(rowptr, col)
rs = np.random.default_rng(5)
qu, qv = rs.integers(0, n, nq).astype(np.int32), rs.integers(0, n, nq).astype(np.int32)
pairs, scores = float(n) * (n - 1) / 2.0, float(nq) * n
out = {"workload": "top_pairs: all pairs of %d nodes, n_emb=%d, k=%d, exclude on (power-law graph, %d edges); rank: %d queries x %d columns, exclude on"
                   % (n, d, k, n_edges, nq, n),
       "pairs": pairs, "rank_scores": scores, "workload_gen_s": t_gen,
       "expectation_text": "time per pair of top_pairs <= %.1f x time per score of Engine.rank in the same run, per precision" % EXPECTED_RATIO,
       "expectation_written_before_the_run": True}
small = np.arange(0, n, max(1, n // 8192), dtype=np.int32)
for p in ("fp32", "bf16"):
    eng.top_pairs(min(k, 1000), nodes=small, precision=p)  # warm-up: a sample of the nodes
    eng.rank(qu[:2048], qv[:2048], precision=p, exclude=True)
    tp_ms, rk_ms, stats, wall = [], [], [], []
    for _ in range(RUNS):  # alternating
        t = time.time()
        res = eng.top_pairs(k, precision=p, exclude=True)
        wall.append(time.time() - t)
        tp_ms.append(res["ms"])
        stats.append(res["stats"])
        rk_ms.append(eng.rank(qu, qv, precision=p, exclude=True)["kernel_ms"])
    best = int(np.argmin(tp_ms))
    t_, r_ = tp_ms[best], min(rk_ms)
    ratio = (t_ / pairs) / (r_ / scores)
    out[p] = {"top_pairs_ms": t_, "top_pairs_runs_ms": tp_ms, "top_pairs_call_s": wall, "rank_ms": r_, "rank_runs_ms": rk_ms,
              "top_pairs_pairs_per_s": pairs / (t_ * 1e-3), "rank_scores_per_s": scores / (r_ * 1e-3),
              "ratio_per_pair_top_pairs_to_rank": ratio,
              "ratio_spread": [(min(tp_ms) / pairs) / (max(rk_ms) / scores), (max(tp_ms) / pairs) / (min(rk_ms) / scores)],
              "expectation_held": bool(ratio <= EXPECTED_RATIO),
              "stats": stats[best], "compaction_share": stats[best]["compaction_ms"] / t_, "n_found": res["n_found"]}
    if p == "fp32":
        f = res["n_found"]
        sub = np.sort(rs.choice(f, min(f, 4096), replace=False))
        rk = eng.rank(res["u"][sub], res["v"][sub], precision="fp32", exclude=False)
        u64, v64 = res["u"][:f].astype(np.int64), res["v"][:f].astype(np.int64)
        known = np.array([np.any(col[rowptr[a]:rowptr[a + 1]] == b) for a, b in zip(u64[sub].tolist(), v64[sub].tolist())])
        s = res["score"][:f].astype(np.float64)
        in_order = bool(np.all((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & ((u64[:-1] < u64[1:]) | ((u64[:-1] == u64[1:]) & (v64[:-1] < v64[1:]))))))
        out["parity_fp32"] = {"sample": int(len(sub)),
                              "score_bits_equal_rank": bool(np.array_equal(rk["score"].view(np.uint32), np.ascontiguousarray(res["score"][sub]).view(np.uint32))),
                              "no_training_edge": bool(not known.any()), "u_below_v": bool((u64 < v64).all()), "in_order": in_order}
eng.close()
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
