#!/usr/bin/env python3
"""Full-ranking link evaluation (gg_rank_scores) on the synthetic power-law workload, beside the streamed top-K
(gg_topk_scores, k = 100) on the SAME row nodes in the same process: the rank stream does strictly less work per tile than
the top-K stream (one threshold per row and a count; no lists, no merge), so the expectation -- measured here, not fixed -- is
rank kernel_ms <= top-K kernel_ms per precision.
    python tools/rank_bench.py [n_node] [n_emb] [n_queries] [k]        (default 10^6 128 65536 100)
One JSON line: per precision kernel_ms (best of 3) and call_s of Engine.rank with exclude off and on, of Engine.topk with
exclude off and on, the ratios rank / top-K, TFLOP/s of the rank stream (2 queries N d), and an at-size consistency leg: the
k-th entry of 4 096 top-K lists, ranked, must come back as rank k with the list's score bits."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import graphgan_amd as ga  # noqa: E402
from graphgan_amd import workloads  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 128
m = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
k = int(sys.argv[4]) if len(sys.argv) > 4 else 100
t0 = time.time()
rowptr, col, emb, n_edges = workloads.powerlaw_workload(n, n_emb=d)
t_gen = time.time() - t0
eng = ga.Engine(emb, emb, optimizer=ga.GG_OPT_SGD)  # SGD: no Adam slots
eng.set_graph_csr(rowptr, col)
rs = np.random.default_rng(5)
u = rs.integers(0, n, m).astype(np.int32)
v = rs.integers(0, n, m).astype(np.int32)
flop = 2.0 * m * n * d
out = {"workload": "full ranking: %d random (u, v) pairs x %d nodes, n_emb=%d (power-law graph, %d edges); top-%d on the same row nodes"
                   % (m, n, d, n_edges, k), "flop": flop, "workload_gen_s": t_gen}


def best_of(fn, reps=3):
    best, wall, res = None, None, None
    for _ in range(reps):
        t = time.time()
        res = fn()
        wall = time.time() - t
        best = res["kernel_ms"] if best is None else min(best, res["kernel_ms"])
    return best, wall, res


for prec, peak in (("fp32", 157.3), ("bf16", 2500.0)):
    leg = {}
    for exclude in (False, True):
        sfx = "_exclude" if exclude else ""
        # alternating, so that both see the same clocks
        r_ms, r_wall, _ = best_of(lambda: eng.rank(u, v, precision=prec, exclude=exclude))
        t_ms, t_wall, _ = best_of(lambda: eng.topk(u, k=k, precision=prec, exclude=exclude))
        r2_ms, _, _ = best_of(lambda: eng.rank(u, v, precision=prec, exclude=exclude), reps=2)
        r_ms = min(r_ms, r2_ms)
        leg.update({"rank%s_kernel_ms" % sfx: r_ms, "rank%s_call_s" % sfx: r_wall, "topk%s_kernel_ms" % sfx: t_ms, "topk%s_call_s" % sfx: t_wall,
                    "rank_over_topk%s" % sfx: r_ms / t_ms})
    tf = flop / (leg["rank_kernel_ms"] * 1e-3) / 1e12
    leg.update({"achieved": tf, "peak": peak, "unit": "TFLOP/s", "frac": tf / peak})
    # consistency at size: the k-th entry of a top-K list has rank k, with the list's score bits
    rows = u[:4096]
    for exclude in (False, True):
        top = eng.topk(rows, k=k, precision=prec, exclude=exclude)
        res = eng.rank(rows, top["col"][:, k - 1], precision=prec, exclude=exclude)
        leg["kth_entry_has_rank_k%s" % ("_exclude" if exclude else "")] = bool(
            (res["rank"] == k).all() and np.array_equal(res["score"].view(np.uint32), np.ascontiguousarray(top["score"][:, k - 1]).view(np.uint32)))
    out[prec] = leg
eng.close()
print(json.dumps(out))
