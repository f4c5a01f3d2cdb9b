#!/usr/bin/env python3
"""The exact silhouette on the device (gg_silhouette) beside the rank consumer of the same tile stream (gg_rank_scores), in the
SAME run, on the table of the 10^6-node synthetic workload:
    silhouette  2^18 random nodes, k = 40 clusters from one kmeans_fit: 2^18 x 2^18 = 6.9 10^10 distances
    rank        65 536 queries over the 10^6 columns:                  6.6 10^10 scores
    python tools/silhouette_bench.py [n_node] [n_emb] [k] [m] [queries] [--out PATH]   (default 10^6 128 40 262144 65536)
One JSON line, also written to PATH (default profiles/r18_silhouette_bench.json).  Both precisions; the legs ALTERNATE, three
runs each, best of 3 (the spread is reported); ms are HIP-event times of the device work (ms_out / kernel_ms): the silhouette's
include its cluster-sorted copy, the row passes and the finish kernels, the rank's its gather and stream kernels.  Per pair the
silhouette costs a correctly rounded square root, two adds and a masked add where the rank costs a compare."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

argv = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "r18_silhouette_bench.json")
if "--out" in argv:
    i = argv.index("--out")
    out_path = argv[i + 1]
    del argv[i:i + 2]
n = int(argv[0]) if len(argv) > 0 else 1_000_000
d = int(argv[1]) if len(argv) > 1 else 128
k = int(argv[2]) if len(argv) > 2 else 40
m = int(argv[3]) if len(argv) > 3 else 1 << 18
nq = int(argv[4]) if len(argv) > 4 else 65536
RUNS = 3

import graphgan_amd as ga  # noqa: E402

# the embedding recipe of workloads.powerlaw_workload and the rows of kmeans_bench.py
emb = np.random.default_rng(5).standard_normal((n, d), dtype=np.float32) * np.float32(0.6 * np.sqrt(50.0 / d))
rs = np.random.default_rng(7)
nodes = rs.choice(n, m, replace=False).astype(np.int32)
start = nodes[rs.choice(m, k, replace=False)]
qu, qv = rs.integers(0, n, nq).astype(np.int32), rs.integers(0, n, nq).astype(np.int32)

eng = ga.Engine(emb, emb, optimizer=ga.GG_OPT_SGD)
fit = eng.kmeans_fit(nodes, k, init=start, max_iters=10)
assign = fit["assign"]
out = {"workload": "silhouette: %d rows of a %d x %d table, k = %d (one kmeans_fit of %d sweeps, %d empty clusters); rank: %d queries x %d columns"
       % (m, n, d, k, fit["iters"], int((fit["counts"] == 0).sum()), nq, n),
       "silhouette_pairs": float(m) * m, "rank_pairs": float(nq) * n}
warm = np.arange(0, m, max(1, m // 2048), dtype=np.int64)
for p in ("fp32", "bf16"):
    eng.silhouette(nodes, assign, k=k, rows=warm, precision=p)  # warm-up: a sample of the rows
    eng.rank(qu[:2048], qv[:2048], precision=p)
    sil_ms, rank_ms = [], []
    for _ in range(RUNS):  # alternating
        res = eng.silhouette(nodes, assign, k=k, precision=p)
        sil_ms.append(res["ms"])
        rank_ms.append(eng.rank(qu, qv, precision=p)["kernel_ms"])
    s, r = min(sil_ms), min(rank_ms)
    out[p] = {"silhouette_ms": s, "silhouette_runs_ms": sil_ms, "rank_ms": r, "rank_runs_ms": rank_ms,
              "silhouette_pairs_per_s": float(m) * m / (s * 1e-3), "rank_pairs_per_s": float(nq) * n / (r * 1e-3),
              "ratio_per_pair_silhouette_to_rank": (s / (float(m) * m)) / (r / (float(nq) * n)),
              "ratio_spread": [(min(sil_ms) / (float(m) * m)) / (max(rank_ms) / (float(nq) * n)), (max(sil_ms) / (float(m) * m)) / (min(rank_ms) / (float(nq) * n))],
              "mean_silhouette": res["mean"]}
# parity of 256 rows against float64 (every column): the largest |sil - float64|
sub = np.sort(rs.choice(m, 256, replace=False)).astype(np.int64)
X = emb[nodes].astype(np.float64)
h = (X * X).sum(axis=1)
dist = np.sqrt(np.maximum(0.0, h[sub][:, None] + h[None, :] - 2.0 * X[sub] @ X.T))
dist[np.arange(256), sub] = 0.0
counts = np.bincount(assign, minlength=k).astype(np.float64)
S = np.stack([dist[:, assign == c].sum(axis=1) for c in range(k)], axis=1)
own = assign[sub]
a = S[np.arange(256), own] / np.maximum(counts[own] - 1, 1)
means = np.where(counts > 0, S / np.maximum(counts, 1), np.inf)
means[np.arange(256), own] = np.inf
b = means.min(axis=1)
want = np.where(counts[own] > 1, (b - a) / np.maximum(a, b), 0.0)
out["parity_fp32_sil_max_abs_diff_256_rows"] = float(np.abs(eng.silhouette(nodes, assign, k=k, rows=sub)["sil"] - want).max())
eng.close()
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
