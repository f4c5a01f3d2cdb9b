#!/usr/bin/env python3
"""Streamed top-K retrieval (gg_topk_scores) at BASELINE.json configs[4] size, beside K7's max-only consumer in the SAME
process (gg_all_score_reduce, logsumexp off: the same tile stream with the cheapest consumer).
    python tools/topk_bench.py [n_node] [n_emb] [n_rows] [k]        (default 10^7 256 4096 100)
One JSON line: per precision kernel_ms (best of 3), call_s, TFLOP/s (2 rows N d, K7's flop count) and its fraction of the
dense MFMA peak; the max-only kernel_ms and the ratio to it; exclude = 1 on the synthetic power-law graph (no target); and a
parity leg on 32 rows (fp32: equal to the oracle's fp32 rows, stably sorted; bf16: fp64 numpy on the bf16-rounded table).
    python tools/topk_bench.py --metric cosine [--metric l2] [n_node] [n_emb] [n_rows] [k]
measures the metric consumer (gg_topk_metric) instead: per precision the dot leg (gg_topk_scores) and every named metric,
ALTERNATING in the same process, best of 3 by HIP events, and each metric's ratio to the dot leg (expected: at most about 1.1)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import graphgan_amd as ga  # noqa: E402
from graphgan_amd import workloads  # noqa: E402

argv, metrics = [], []
for i, a in enumerate(sys.argv[1:], 1):
    if a == "--metric":
        metrics.append(sys.argv[i + 1])
    elif sys.argv[i - 1] != "--metric":
        argv.append(a)
if any(m not in ("cosine", "l2", "dot") for m in metrics):
    sys.exit("--metric must be cosine, l2 or dot")
n = int(argv[0]) if len(argv) > 0 else 10_000_000
d = int(argv[1]) if len(argv) > 1 else 256
r = int(argv[2]) if len(argv) > 2 else 4096
k = int(argv[3]) if len(argv) > 3 else 100
t0 = time.time()
rowptr, col, emb, n_edges = workloads.powerlaw_workload(n, n_emb=d)
t_gen = time.time() - t0
eng = ga.Engine(emb, emb, optimizer=ga.GG_OPT_SGD)  # SGD: no Adam slots (the tables alone are 2 x 10 GB)
eng.set_graph_csr(rowptr, col)
rs = np.random.default_rng(5)
rows = np.sort(rs.choice(n, r, replace=False)).astype(np.int32)
flop = 2.0 * r * n * d
out = {"workload": "top-%d retrieval: %d rows x %d nodes, n_emb=%d (power-law graph, %d edges)" % (k, r, n, d, n_edges), "flop": flop,
       "workload_gen_s": t_gen}


def best_of(fn, reps=3):
    best, wall, res = None, None, None
    for _ in range(reps):
        t = time.time()
        res = fn()
        wall = time.time() - t
        best = res["kernel_ms"] if best is None else min(best, res["kernel_ms"])
    return best, wall, res


if metrics:
    # the metric legs beside the dot leg: one round = every leg once, three rounds, the best kernel_ms of each leg
    legs = ["dot"] + [m for m in metrics if m != "dot"]
    for prec in ("fp32", "bf16"):
        eng.topk(rows[:64], k=k, precision=prec)  # (the bf16 copy's first build, the kernels' first load)
        runs = {m: [] for m in legs}
        for _ in range(3):
            for m in legs:
                runs[m].append(eng.topk(rows, k=k, precision=prec, metric=m)["kernel_ms"])
        out[prec] = {m: {"kernel_ms": min(v), "runs_ms": v, "ratio_to_dot": min(v) / min(runs["dot"])} for m, v in runs.items()}
        out[prec]["expected_ratio_at_most"] = 1.1
    eng.close()
    print(json.dumps(out))
    sys.exit(0)

for prec, peak in (("fp32", 157.3), ("bf16", 2500.0)):
    ref_ms, _, _ = best_of(lambda: eng.all_score_reduce(rows, precision=prec, logsumexp=False))
    ms, wall, res = best_of(lambda: eng.topk(rows, k=k, precision=prec))
    ms_x, wall_x, _ = best_of(lambda: eng.topk(rows, k=k, precision=prec, exclude=True), reps=2)
    tf = flop / (ms * 1e-3) / 1e12
    out[prec] = {"kernel_ms": ms, "call_s": wall, "achieved": tf, "peak": peak, "unit": "TFLOP/s", "frac": tf / peak,
                 "all_score_reduce_max_only_kernel_ms": ref_ms, "ratio_to_max_only": ms / ref_ms,
                 "target_ratio": 1.25 if prec == "fp32" else 1.5,
                 "exclude_kernel_ms": ms_x, "exclude_call_s": wall_x, "exclude_ratio_to_max_only": ms_x / ref_ms}

# parity on 32 rows
from oracle import graphgan_oracle as orc  # noqa: E402


def bf16_round(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32)).view(np.float32)


prow = rows[:: max(1, r // 32)][:32]
got = eng.topk(prow, k=k, precision="fp32")
from concurrent.futures import ThreadPoolExecutor  # noqa: E402
zeros = np.zeros(n, np.float32)
E_pad = emb if d % 4 == 0 else orc.pad_rows(emb)
with ThreadPoolExecutor(16) as pool:  # (one oracle row per call; ctypes releases the GIL)
    S = np.concatenate(list(pool.map(lambda u: orc.c_all_score_rows(E_pad, zeros, np.array([u], np.int32)), prow.tolist())))
o = np.zeros((len(prow), k), np.int64)
for i in range(len(prow)):  # (stable sort of the row, restricted to the scores at or above its k-th largest)
    c = np.flatnonzero(S[i] >= np.partition(S[i], n - k)[n - k])
    o[i] = c[np.lexsort((c, -S[i, c]))][:k]
out["parity_fp32_32rows_equal"] = bool(np.array_equal(got["col"], o) and np.array_equal(got["score"], np.take_along_axis(S, o, 1)))
del S
gotb = eng.topk(prow, k=k, precision="bf16")
A = bf16_round(emb[prow]).astype(np.float64)
top_s = []
smax = 0.0
for c0 in range(0, n, 1 << 20):
    Sb = A @ bf16_round(emb[c0:c0 + (1 << 20)]).astype(np.float64).T
    smax = max(smax, float(np.abs(Sb).max()))
    top_s.append(-np.sort(-Sb, axis=1)[:, :k])
ref = -np.sort(-np.concatenate(top_s, 1), axis=1)[:, :k]
out["parity_bf16_32rows_max_abs_score_diff"] = float(np.max(np.abs(gotb["score"] - ref)))
out["parity_bf16_tolerance"] = 2e-3 * max(1.0, smax)
eng.close()
print(json.dumps(out))
