#!/usr/bin/env python3
"""The node-classification fit (gg_classifier_fit) on the table of the 10^6-node synthetic workload, beside an unfused torch
fp32 evaluation of the same loss and gradient on the same rows in the SAME run: behind the engine's legs this script starts
itself once more with --torch-leg (a fresh child process: torch ships a HIP runtime of its own, and two HIP runtimes do not share
one process) and reads the child's time.  A baseline that cannot run fails the tool: there is no result without it.
    python tools/classifier_bench.py [n_node] [n_emb] [n_class] [m]        (default 10^6 128 40 900000)
    python tools/classifier_bench.py --engine-only ...                     (the engine's legs alone, for a profiler)
    python tools/classifier_bench.py --multilabel ...                      (also the one-vs-rest fit, gg_classifier_ml_fit, in the same run)
One JSON line: ms per iteration of a fit (sweep + stage reduction + Adam: HIP events around the enqueued iterations, divided by
their number -- an upper bound of the sweep alone), ms per fit of the default 200 iterations, the fractions of the HBM model
(m d 4 B per sweep at 8 TB/s) and of the flop model (4 m d C per sweep at the 155 TFLOP/s that v_mfma_f32_32x32x2_f32 sustains on
the MI355X: 157.3 TFLOP/s by specification, 64 cycles per SIMD and instruction), the torch baseline (index_select, two matmuls, one
softmax; best of 5, torch.cuda events) and the ratio to it, and a parity leg against float64 numpy on 4 096 of the rows.
With --multilabel the same rows get 1-3 labels each and the sigmoid variant of the sweep is timed the same way (3 warm-up
iterations, best of 3 x 20) beside the softmax variant: ml_ms_per_iteration, the ratio of the two, and its own parity leg."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

flags = [a for a in sys.argv[1:] if a.startswith("--")]
args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 1_000_000
d = int(args[1]) if len(args) > 1 else 128
C = int(args[2]) if len(args) > 2 else 40
m = int(args[3]) if len(args) > 3 else 900_000
HBM_TBS, MFMA_F32_TFLOPS = 8.0, 155.0

# the embedding recipe of workloads.powerlaw_workload (the fit reads no graph)
emb = np.random.default_rng(5).standard_normal((n, d), dtype=np.float32) * np.float32(0.6 * np.sqrt(50.0 / d))
rs = np.random.default_rng(7)
nodes = rs.choice(n, m, replace=False).astype(np.int32)
labels = rs.integers(0, C, m).astype(np.int32)
W = (0.1 * rs.standard_normal((C, d))).astype(np.float32)
b = (0.1 * rs.standard_normal(C)).astype(np.float32)


def torch_leg():
    """best-of-5 ms of one unfused loss-and-gradient evaluation: index_select, two matmuls, one softmax (torch.cuda events)"""
    import torch
    dev = torch.device("cuda")
    E_t = torch.from_numpy(emb).to(dev)
    idx = torch.from_numpy(nodes.astype(np.int64)).to(dev)
    y_t = torch.from_numpy(labels.astype(np.int64)).to(dev)
    W_t, b_t = torch.from_numpy(W).to(dev), torch.from_numpy(b).to(dev)
    rows = torch.arange(m, device=dev)

    def lossgrad():
        X_t = E_t.index_select(0, idx)
        lp = torch.log_softmax(X_t @ W_t.T + b_t, dim=1)
        loss = -lp.gather(1, y_t[:, None]).mean()
        P = lp.exp()
        P[rows, y_t] -= 1.0
        return loss, P.T @ X_t / m, P.sum(0) / m

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
    return {"ms": best, "loss": float(res[0]), "torch": torch.__version__}


if "--torch-leg" in flags:
    print(json.dumps(torch_leg()))
    sys.exit(0)

import graphgan_amd as ga  # noqa: E402

eng = ga.Engine(emb, emb, optimizer=ga.GG_OPT_SGD)

eng.classifier_fit(nodes, labels, C, iters=3)  # warm-up
it_ms = min(eng.classifier_fit(nodes, labels, C, iters=20)["ms"] / 20 for _ in range(3))
fit = eng.classifier_fit(nodes, labels, C, iters=200)
out = {"workload": "softmax regression: %d rows of a %d x %d table, %d classes" % (m, n, d, C),
       "ms_per_iteration": it_ms, "ms_per_sweep_upper_bound": it_ms, "ms_per_fit_200": fit["ms"],
       "loss_first": float(fit["loss"][0]), "loss_last": float(fit["loss"][-1]),
       "hbm_model_ms": m * d * 4 / (HBM_TBS * 1e12) * 1e3, "flop_model_ms": 4.0 * m * d * C / (MFMA_F32_TFLOPS * 1e12) * 1e3}
out["frac_hbm_model"] = out["hbm_model_ms"] / it_ms
out["frac_flop_model"] = out["flop_model_ms"] / it_ms
out["padded_flop_note"] = "the kernel pads C to %d (32-class tiles): %.2f of its matrix work is the model's" % (-(-C // 32) * 32, C / (-(-C // 32) * 32))

# parity on 4 096 rows at non-zero parameters
sub = slice(0, 4096)
got = eng.classifier_lossgrad(nodes[sub], labels[sub], W, b, l2=1e-4)
X = emb[nodes[sub]].astype(np.float64)
z = X @ W.astype(np.float64).T + b
z -= z.max(axis=1, keepdims=True)
p = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)
p[np.arange(4096), labels[sub]] -= 1.0
out["parity_gW_max_abs_diff"] = float(np.max(np.abs(got["gW"] - (p.T @ X / 4096 + 1e-4 * W))))
out["loss_at_parity_params"] = float(eng.classifier_lossgrad(nodes, labels, W, b)["loss"])
if "--multilabel" in flags:
    Y = np.zeros((m, C), dtype=bool)
    Y[np.arange(m), labels] = True
    for extra in range(2):  # a second and a third label on a third of the rows each (a draw that repeats a label adds none)
        pick = rs.random(m) < 1.0 / 3.0
        Y[np.flatnonzero(pick), rs.integers(0, C, int(pick.sum()))] = True
    from graphgan_amd.engine import pack_label_bits
    bits = pack_label_bits(Y, C)
    eng.classifier_ml_fit(nodes, bits, C, iters=3)  # warm-up
    ml_ms = min(eng.classifier_ml_fit(nodes, bits, C, iters=20)["ms"] / 20 for _ in range(3))
    ml_fit = eng.classifier_ml_fit(nodes, bits, C, iters=200)
    got = eng.classifier_ml_lossgrad(nodes[sub], bits[sub], W, b, l2=1e-4)
    z = X @ W.astype(np.float64).T + b
    e = np.exp(-np.abs(z))
    p = np.where(z >= 0, 1.0, e) / (1.0 + e) - Y[sub]
    out.update({"ml_workload": "one-vs-rest logistic regression on the same rows, %.2f labels per row" % Y.sum(axis=1).mean(),
                "ml_ms_per_iteration": ml_ms, "ml_ms_per_fit_200": ml_fit["ms"], "ml_loss_first": float(ml_fit["loss"][0]),
                "ml_loss_last": float(ml_fit["loss"][-1]), "ratio_ml_to_softmax_iteration": ml_ms / it_ms,
                "ml_parity_gW_max_abs_diff": float(np.max(np.abs(got["gW"] - (p.T @ X / 4096 + 1e-4 * W)))),
                "ml_parity_loss_abs_diff": abs(got["loss"] - float((np.maximum(z, 0) + np.log1p(e) - Y[sub] * z).sum() / 4096
                                                                   + 0.5e-4 * (W.astype(np.float64) ** 2).sum()))})
eng.close()
if "--engine-only" not in flags:
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-leg"] + args, capture_output=True, text=True)
    if child.returncode != 0:
        sys.exit("classifier_bench: the torch baseline failed, no result:\n" + child.stderr[-2000:])
    leg = json.loads(child.stdout.strip().splitlines()[-1])
    out["torch_unfused_ms"] = leg["ms"]
    out["torch_version"] = leg["torch"]
    out["torch_loss_same_rows"] = leg["loss"]
    out["ratio_fused_iteration_to_torch"] = it_ms / leg["ms"]
print(json.dumps(out))
