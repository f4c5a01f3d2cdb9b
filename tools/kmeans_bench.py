#!/usr/bin/env python3
"""A Lloyd iteration of the on-device k-means (gg_kmeans_fit) on the table of the 10^6-node synthetic workload, beside the
softmax iteration of gg_classifier_fit at C = k and an unfused torch fp32 evaluation of one Lloyd iteration (index_select, cdist,
argmin, index_add_), all on the same rows in the SAME run.  The torch leg is a fresh child process (--torch-leg), as in
classifier_bench.py: two HIP runtimes do not share one process.  A baseline that cannot run fails the tool.
    python tools/kmeans_bench.py [n_node] [n_emb] [k] [m]        (default 10^6 128 40 900000)
    python tools/kmeans_bench.py --engine-only ...               (the engine's legs alone, for a profiler)
One JSON line.  ms per Lloyd iteration (sweep + update: HIP events around the enqueued iterations, ms_out, divided by the sweeps
that ran) from a fit of ITERS sweeps started on k random rows -- Gaussian rows have no cluster structure, so the fit does not
converge early (asserted).  The softmax iteration (sweep + reduction + Adam) is timed the same way.  The two fits ALTERNATE, three
runs each: the margin of the comparison is the spread of those runs.  Byte model: m d 4 B per sweep at 8 TB/s; flop model:
4 m d k per sweep at the 155 TFLOP/s that v_mfma_f32_32x32x2_f32 sustains on the MI355X.  A parity leg checks one sweep against
float64 numpy on 4 096 of the rows."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

flags = [a for a in sys.argv[1:] if a.startswith("--")]
args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 1_000_000
d = int(args[1]) if len(args) > 1 else 128
k = int(args[2]) if len(args) > 2 else 40
m = int(args[3]) if len(args) > 3 else 900_000
ITERS = 20
HBM_TBS, MFMA_F32_TFLOPS = 8.0, 155.0

# the embedding recipe of workloads.powerlaw_workload and the rows of classifier_bench.py (neither fit reads a graph)
emb = np.random.default_rng(5).standard_normal((n, d), dtype=np.float32) * np.float32(0.6 * np.sqrt(50.0 / d))
rs = np.random.default_rng(7)
nodes = rs.choice(n, m, replace=False).astype(np.int32)
labels = rs.integers(0, k, m).astype(np.int32)
start = nodes[rs.choice(m, k, replace=False)]


def torch_leg():
    """best-of-5 ms of one unfused Lloyd iteration: index_select, cdist, argmin, index_add_, bincount, the division"""
    import torch
    dev = torch.device("cuda")
    E_t = torch.from_numpy(emb).to(dev)
    idx = torch.from_numpy(nodes.astype(np.int64)).to(dev)
    C_t = E_t.index_select(0, torch.from_numpy(start.astype(np.int64)).to(dev)).clone()

    def lloyd(C):
        X_t = E_t.index_select(0, idx)
        D = torch.cdist(X_t, C)
        dist, a = D.min(dim=1)
        sums = torch.zeros_like(C).index_add_(0, a, X_t)
        counts = torch.bincount(a, minlength=k)
        new = torch.where(counts[:, None] > 0, sums / counts.clamp(min=1)[:, None], C)
        return new, (dist * dist).sum()

    for _ in range(3):
        lloyd(C_t)
    torch.cuda.synchronize()
    best = None
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = lloyd(C_t)
        e1.record()
        torch.cuda.synchronize()
        t = e0.elapsed_time(e1)
        best = t if best is None else min(best, t)
    return {"ms": best, "inertia": float(res[1]), "torch": torch.__version__}


if "--torch-leg" in flags:
    print(json.dumps(torch_leg()))
    sys.exit(0)

import graphgan_amd as ga  # noqa: E402

eng = ga.Engine(emb, emb, optimizer=ga.GG_OPT_SGD)

eng.kmeans_fit(nodes, k, init=start, max_iters=3)  # warm-up
eng.classifier_fit(nodes, labels, k, iters=3)
km_runs, nc_runs = [], []
for _ in range(3):  # alternating
    fit = eng.kmeans_fit(nodes, k, init=start, max_iters=ITERS)
    assert fit["iters"] == ITERS and not fit["converged"], "the start converged early: no fixed number of sweeps was timed"
    km_runs.append(fit["ms"] / fit["iters"])
    nc_runs.append(eng.classifier_fit(nodes, labels, k, iters=ITERS)["ms"] / ITERS)
it_ms, nc_ms = min(km_runs), min(nc_runs)
step_ms = []
for sums in (True, False):  # one sweep, with and without the second product (wall clock of the call: uploads and read-backs included)
    eng.kmeans_step(nodes, centroid_nodes=start, sums=sums)
    t0 = time.perf_counter()
    eng.kmeans_step(nodes, centroid_nodes=start, sums=sums)
    step_ms.append((time.perf_counter() - t0) * 1e3)
out = {"workload": "k-means: %d rows of a %d x %d table, k = %d, %d sweeps from %d random rows" % (m, n, d, k, ITERS, k),
       "ms_per_lloyd_iteration": it_ms, "lloyd_runs_ms": km_runs, "softmax_ms_per_iteration": nc_ms, "softmax_runs_ms": nc_runs,
       "ratio_lloyd_to_softmax_iteration": it_ms / nc_ms,
       "ratio_spread": [min(km_runs) / max(nc_runs), max(km_runs) / min(nc_runs)],
       "inertia_first": float(fit["inertia"][0]), "inertia_last": float(fit["inertia"][-1]), "empty_clusters": int((fit["counts"] == 0).sum()),
       "step_call_wall_ms_with_sums": step_ms[0], "step_call_wall_ms_assign_only": step_ms[1],
       "hbm_model_ms": m * d * 4 / (HBM_TBS * 1e12) * 1e3, "flop_model_ms": 4.0 * m * d * k / (MFMA_F32_TFLOPS * 1e12) * 1e3}
out["frac_hbm_model"] = out["hbm_model_ms"] / it_ms
out["frac_flop_model"] = out["flop_model_ms"] / it_ms
out["padded_flop_note"] = "the kernel pads k to %d (32-cluster tiles): %.2f of its matrix work is the model's" % (-(-k // 32) * 32, k / (-(-k // 32) * 32))

# parity of one sweep on 4 096 rows against float64
sub = nodes[:4096]
C = emb[start]
got = eng.kmeans_step(sub, centroids=C)
X64, C64 = emb[sub].astype(np.float64), C.astype(np.float64)
D = (X64 * X64).sum(axis=1)[:, None] - 2.0 * X64 @ C64.T + (C64 * C64).sum(axis=1)[None, :]
own = D[np.arange(4096), got["assign"]]
out["parity_argmin_excess_max"] = float((own - D.min(axis=1)).max())
out["parity_dist2_max_abs_diff"] = float(np.abs(got["dist2"] - own).max())
out["parity_rows_off_the_float64_argmin"] = int((got["assign"] != D.argmin(axis=1)).sum())
eng.close()
if "--engine-only" not in flags:
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-leg"] + args, capture_output=True, text=True)
    if child.returncode != 0:
        sys.exit("kmeans_bench: the torch baseline failed, no result:\n" + child.stderr[-2000:])
    leg = json.loads(child.stdout.strip().splitlines()[-1])
    out["torch_unfused_ms"] = leg["ms"]
    out["torch_version"] = leg["torch"]
    out["torch_inertia_first_sweep"] = leg["inertia"]
    out["ratio_lloyd_iteration_to_torch"] = it_ms / leg["ms"]
print(json.dumps(out))
