#!/usr/bin/env python3
"""The centred Gram sweep (gg_gram) on the table of the 10^6-node synthetic workload -- the shape of kmeans_bench.py: 9 x 10^5
random rows of a 10^6 x 128 table -- beside a Lloyd iteration of gg_kmeans_fit at k = 40 on the same rows and an unfused torch
fp32 evaluation (index_select, X.T @ X), all in the SAME run.  The torch leg is a fresh child process (--torch-leg), as in
kmeans_bench.py: two HIP runtimes do not share one process.  A baseline that cannot run fails the tool.
    python tools/gram_bench.py [n_node] [n_emb] [k] [m]        (default 10^6 128 40 900000)
    python tools/gram_bench.py --engine-only ...               (the engine's legs alone, for a profiler)
One JSON line.  Every time is a HIP-event time of the device work (ms_out): the sums-only sweep (the mean pass), the full sweep
about the fp32 mean, and a Lloyd iteration (sweep + update, a fit of ITERS sweeps divided by the sweeps that ran).  The three legs
ALTERNATE, three runs each: the margin of a comparison is the spread of those runs.  Byte model: m d 4 B per sweep at 8 TB/s; flop
model: ceil(m / 64) x T x 32 matrix instructions of 4 096 flop (T = DT (DT + 1) / 2 upper output tiles, DT = ceil(d / 32)) at the
155 TFLOP/s that v_mfma_f32_32x32x2_f32 sustains on the MI355X.  EXPECTATION, stated and not gated: the full sweep costs no more
than the Lloyd iteration on the same rows (at d = 128, k = 40 it issues 320 matrix instructions per tile against 512, and both
gather the same bytes).  A parity leg checks one sweep against float64 numpy on 4 096 of the rows."""
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
k = int(args[2]) if len(args) > 2 else 40
m = int(args[3]) if len(args) > 3 else 900_000
ITERS = 20
HBM_TBS, MFMA_F32_TFLOPS = 8.0, 155.0

# the embedding recipe of workloads.powerlaw_workload and the rows of kmeans_bench.py
emb = np.random.default_rng(5).standard_normal((n, d), dtype=np.float32) * np.float32(0.6 * np.sqrt(50.0 / d))
rs = np.random.default_rng(7)
nodes = rs.choice(n, m, replace=False).astype(np.int32)
rs.integers(0, k, m)  # (kmeans_bench.py draws its labels here: the same start rows)
start = nodes[rs.choice(m, k, replace=False)]


def torch_leg():
    """best-of-5 ms of the unfused Gram matrix: index_select, X.T @ X, the column sums"""
    import torch
    dev = torch.device("cuda")
    E_t = torch.from_numpy(emb).to(dev)
    idx = torch.from_numpy(nodes.astype(np.int64)).to(dev)

    def gram():
        X_t = E_t.index_select(0, idx)
        return X_t.T @ X_t, X_t.sum(dim=0)

    for _ in range(3):
        gram()
    torch.cuda.synchronize()
    best = None
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = gram()
        e1.record()
        torch.cuda.synchronize()
        t = e0.elapsed_time(e1)
        best = t if best is None else min(best, t)
    return {"ms": best, "trace": float(res[0].diagonal().sum()), "torch": torch.__version__}


if "--torch-leg" in flags:
    print(json.dumps(torch_leg()))
    sys.exit(0)

import graphgan_amd as ga  # noqa: E402

eng = ga.Engine(emb, emb, optimizer=ga.GG_OPT_SGD)

mean = (eng.gram(nodes, gram=False)["sums"] / m).astype(np.float32)  # warm-up of every leg
eng.gram(nodes, center=mean)
eng.kmeans_fit(nodes, k, init=start, max_iters=3)
sums_runs, full_runs, km_runs = [], [], []
for _ in range(3):  # alternating
    sums_runs.append(eng.gram(nodes, gram=False)["ms"])
    full = eng.gram(nodes, center=mean)
    full_runs.append(full["ms"])
    fit = eng.kmeans_fit(nodes, k, init=start, max_iters=ITERS)
    assert fit["iters"] == ITERS and not fit["converged"], "the start converged early: no fixed number of sweeps was timed"
    km_runs.append(fit["ms"] / fit["iters"])
DT = -(-d // 32)
T = DT * (DT + 1) // 2
tiles = -(-m // 64)
out = {"workload": "Gram sweep: %d rows of a %d x %d table; Lloyd iteration at k = %d on the same rows" % (m, n, d, k),
       "gram_sums_only_ms": min(sums_runs), "gram_sums_only_runs_ms": sums_runs, "gram_full_ms": min(full_runs), "gram_full_runs_ms": full_runs,
       "ms_per_lloyd_iteration": min(km_runs), "lloyd_runs_ms": km_runs,
       "ratio_full_sweep_to_lloyd_iteration": min(full_runs) / min(km_runs),
       "ratio_spread": [min(full_runs) / max(km_runs), max(full_runs) / min(km_runs)],
       "expectation_full_sweep_no_more_than_lloyd_iteration_held": bool(min(full_runs) <= min(km_runs)),
       "grid": min(ga._lib.GRAM_MAX_GRID, tiles), "upper_output_tiles": T, "matrix_instructions_per_tile": 32 * T,
       "lloyd_matrix_instructions_per_tile": 2 * 32 * (-(-k // 32)) * DT,
       "hbm_model_ms": m * d * 4 / (HBM_TBS * 1e12) * 1e3, "flop_model_ms": tiles * T * 32 * 4096.0 / (MFMA_F32_TFLOPS * 1e12) * 1e3,
       "residual_sums_max_abs": float(np.abs(full["sums"]).max())}
out["frac_hbm_model_sums_only"] = out["hbm_model_ms"] / out["gram_sums_only_ms"]
out["frac_hbm_model_full"] = out["hbm_model_ms"] / out["gram_full_ms"]
out["frac_flop_model_full"] = out["flop_model_ms"] / out["gram_full_ms"]

# parity of one sweep on 4 096 rows against float64, in units of the derived band (m + 3) 2^-24 sum_i |C_ij| |C_il|
sub = nodes[:4096]
got = eng.gram(sub, center=mean)
C = emb[sub].astype(np.float64) - mean.astype(np.float64)
A = np.abs(C)
out["parity_gram_err_over_band_max"] = float((np.abs(got["gram"] - C.T @ C) / ((4096 + 3) * 2.0 ** -24 * (A.T @ A))).max())
out["parity_sums_err_over_band_max"] = float((np.abs(got["sums"] - C.sum(axis=0)) / ((4096 + 1) * 2.0 ** -24 * A.sum(axis=0))).max())
eng.close()
if "--engine-only" not in flags:
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-leg"] + args, capture_output=True, text=True)
    if child.returncode != 0:
        sys.exit("gram_bench: the torch baseline failed, no result:\n" + child.stderr[-2000:])
    leg = json.loads(child.stdout.strip().splitlines()[-1])
    out["torch_unfused_ms"] = leg["ms"]
    out["torch_version"] = leg["torch"]
    out["torch_trace_uncentred"] = leg["trace"]
    out["ratio_full_sweep_to_torch"] = out["gram_full_ms"] / leg["ms"]
print(json.dumps(out))
