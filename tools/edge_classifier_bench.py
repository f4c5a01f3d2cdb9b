#!/usr/bin/env python3
"""The learned link-prediction fit (gg_edge_classifier_fit) on random pairs of the table of the 10^6-node synthetic workload,
for each of the four operators, beside an unfused torch fp32 evaluation of the same loss and gradient on the same pairs in the
SAME run.  Behind the engine's legs this script starts itself twice more, each time as a fresh child process:
  --torch-leg   the torch baseline (torch ships a HIP runtime of its own, and two HIP runtimes do not share one process);
  --trace-leg   the fits alone under `rocprofv3 --kernel-trace --stats`, for the split of an iteration into its three kernels.
A leg that cannot run fails the tool: there is no result without it.
    python tools/edge_classifier_bench.py [n_node] [n_emb] [m]        (default 10^6 128 10^6)
    python tools/edge_classifier_bench.py --engine-only ...           (the engine's legs alone)
One JSON line.  Per operator: ms per iteration of a fit (HIP events around 20 enqueued iterations, divided by their number; 3
warm-up iterations, best of 3), the mean ms per dispatch of edge_sweep_kernel by the kernel trace, the fractions of the HBM
model -- two rows of ld floats per edge and iteration, 2 ld 4 m bytes, at the 8 TB/s of the specification and at the 6.29 TB/s a
float4 copy reaches on the MI355X --, the torch baseline (two index_selects, the operator, a matrix-vector product each way;
best of 5, torch.cuda events), the ratio to it, both losses, and a parity leg against float64 numpy on 4 096 of the pairs.
nc_reduce_kernel and nc_adam_kernel are shared by the operators: their mean ms per dispatch is reported once."""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

flags = [a for a in sys.argv[1:] if a.startswith("--")]
args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 1_000_000
d = int(args[1]) if len(args) > 1 else 128
m = int(args[2]) if len(args) > 2 else 1_000_000
HBM_TBS, COPY_TBS = 8.0, 6.29
OPS = ("hadamard", "average", "l1", "l2")

# the embedding recipe of workloads.powerlaw_workload (the fit reads no graph)
emb = np.random.default_rng(5).standard_normal((n, d), dtype=np.float32) * np.float32(0.6 * np.sqrt(50.0 / d))
rs = np.random.default_rng(7)
u = rs.integers(0, n, m).astype(np.int32)
v = rs.integers(0, n, m).astype(np.int32)
y = rs.integers(0, 2, m).astype(np.int32)
w = (0.1 * rs.standard_normal(d)).astype(np.float32)
b = np.float32(0.1)


def features(A, B, op, xp):
    if op == "hadamard":
        return A * B
    if op == "average":
        return (A + B) * 0.5
    if op == "l1":
        return xp.abs(A - B)
    return (A - B) * (A - B)


def torch_leg():
    """per operator the best-of-5 ms of one unfused loss-and-gradient evaluation (torch.cuda events) and its loss"""
    import torch
    dev = torch.device("cuda")
    E_t = torch.from_numpy(emb).to(dev)
    iu, iv = torch.from_numpy(u.astype(np.int64)).to(dev), torch.from_numpy(v.astype(np.int64)).to(dev)
    y_t = torch.from_numpy(y.astype(np.float32)).to(dev)
    w_t, b_t = torch.from_numpy(w).to(dev), float(b)
    out = {"torch": torch.__version__}
    for op in OPS:
        def lossgrad():
            X = features(E_t.index_select(0, iu), E_t.index_select(0, iv), op, torch)
            z = X @ w_t + b_t
            loss = (torch.nn.functional.softplus(z) - y_t * z).mean()
            p = torch.sigmoid(z) - y_t
            return loss, p @ X / m, p.sum() / m

        for _ in range(3):
            lossgrad()
        torch.cuda.synchronize()
        best = None
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = lossgrad()
            e1.record()
            torch.cuda.synchronize()
            t = e0.elapsed_time(e1)
            best = t if best is None else min(best, t)
        out[op] = {"ms": best, "loss": float(res[0])}
    return out


if "--torch-leg" in flags:
    print(json.dumps(torch_leg()))
    sys.exit(0)

import graphgan_amd as ga  # noqa: E402

eng = ga.Engine(emb, emb, optimizer=ga.GG_OPT_SGD)
ld = -(-d // 4) * 4


def timed_fits(op):
    eng.edge_classifier_fit(u, v, y, op=op, iters=3)  # warm-up
    return min(eng.edge_classifier_fit(u, v, y, op=op, iters=20)["ms"] / 20 for _ in range(3))


if "--trace-leg" in flags:
    for op in OPS:
        timed_fits(op)
    eng.close()
    sys.exit(0)

bytes_per_iteration = 2.0 * ld * 4 * m
out = {"workload": "logistic regression on op(E[u], E[v]): %d random pairs of a %d x %d table" % (m, n, d),
       "bytes_per_iteration": bytes_per_iteration, "hbm_model_ms": bytes_per_iteration / (HBM_TBS * 1e12) * 1e3,
       "copy_bw_model_ms": bytes_per_iteration / (COPY_TBS * 1e12) * 1e3, "operators": {}}
sub = slice(0, 4096)
A, B = emb[u[sub]].astype(np.float64), emb[v[sub]].astype(np.float64)
for op in OPS:
    it_ms = timed_fits(op)
    fit = eng.edge_classifier_fit(u, v, y, op=op, iters=200)
    r = {"ms_per_iteration": it_ms, "ms_per_fit_200": fit["ms"], "loss_first": float(fit["loss"][0]), "loss_last": float(fit["loss"][-1]),
         "frac_hbm_model": out["hbm_model_ms"] / it_ms, "frac_copy_bw": out["copy_bw_model_ms"] / it_ms,
         "gather_tb_per_s": bytes_per_iteration / (it_ms * 1e-3) / 1e12}
    got = eng.edge_classifier_lossgrad(u[sub], v[sub], y[sub], w, b, op=op, l2=1e-4)
    X = features(A, B, op, np)
    z = X @ w.astype(np.float64) + float(b)
    e = np.exp(-np.abs(z))
    p = np.where(z >= 0, 1.0, e) / (1.0 + e) - y[sub]
    r["parity_gw_max_abs_diff"] = float(np.max(np.abs(got["gw"] - (p @ X / 4096 + 1e-4 * w))))
    r["parity_loss_abs_diff"] = abs(got["loss"] - float((np.maximum(z, 0) + np.log1p(e) - y[sub] * z).sum() / 4096 + 0.5e-4 * (w.astype(np.float64) ** 2).sum()))
    r["loss_at_parity_params"] = float(eng.edge_classifier_lossgrad(u, v, y, w, b, op=op)["loss"])
    out["operators"][op] = r
eng.close()


def child(cmd, what):
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        sys.exit("edge_classifier_bench: %s failed, no result:\n%s" % (what, (res.stdout + res.stderr)[-2000:]))
    return res.stdout


if "--engine-only" not in flags:
    leg = json.loads(child([sys.executable, os.path.abspath(__file__), "--torch-leg"] + args, "the torch baseline").strip().splitlines()[-1])
    out["torch_version"] = leg["torch"]
    for op in OPS:
        r = out["operators"][op]
        r["torch_unfused_ms"] = leg[op]["ms"]
        r["torch_loss_same_pairs"] = leg[op]["loss"]
        r["ratio_iteration_to_torch"] = r["ms_per_iteration"] / leg[op]["ms"]
    with tempfile.TemporaryDirectory() as tmp:
        child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "ec", "--", sys.executable,
               os.path.abspath(__file__), "--trace-leg"] + args, "the kernel trace")
        stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            sys.exit("edge_classifier_bench: the kernel trace wrote no kernel_stats.csv, no result")
        rows = list(csv.DictReader(open(stats[0])))
    mean_ms = lambda key: [(x["Name"], float(x["AverageNs"]) * 1e-6, int(x["Calls"])) for x in rows if key in x["Name"]]  # noqa: E731
    for name, ms, calls in mean_ms("edge_sweep_kernel"):
        op = OPS[int(name.split("edge_sweep_kernel<")[1].split(",")[0])]
        out["operators"][op].update({"sweep_ms": ms, "sweep_dispatches": calls, "sweep_frac_hbm_model": out["hbm_model_ms"] / ms,
                                     "sweep_frac_copy_bw": out["copy_bw_model_ms"] / ms})
    for key in ("nc_reduce_kernel", "nc_adam_kernel"):
        (_, ms, calls), = mean_ms(key)
        out[key[3:-7] + "_ms"] = ms
        out[key[3:-7] + "_dispatches"] = calls
    out["split_source"] = "rocprofv3 --kernel-trace --stats of the fits alone (--trace-leg): mean ms per dispatch"
print(json.dumps(out))
