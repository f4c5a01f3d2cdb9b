#!/usr/bin/env python3
"""Skip-gram pre-training rows (gg_prepare_pretrain) on the bench graph.
    python tools/pretrain_bench.py [n_node] [n_starts] [epoch]        (default 10^6 65536; "epoch": see below)
Setup: the power-law bench graph (m = 10: ~10^7 edges, d = 128), noise weights round(16 max(deg, 1)^0.75), n_starts starts x
10 walks x 40 nodes, window 5, 5 negatives.  One JSON line: rows/s of the call (wall, best of 3), HIP-event times of the walk
and the fill kernel (best of 3), the fill kernel's byte model and its fraction of the 6.29 TB/s float4-copy ceiling, the time
of one fused gg_d_pass over the same rows (batch 4096, lazy Adam), the ratio prepare / d_pass and the link-prediction accuracy
of default-knob pre-training on CA-GrQc.  The node2vec leg ("biased"), same run and same starts: the HIP-event time of the
biased walk kernel for (p, q) = (0.25, 4) and (4, 0.25) beside the uniform one and the fill kernel of the same call, the share
of biased hops that exhausted the 32 rejection trials and took the exact draw (estimated on the host: the numpy oracle of
tests/support/pretrain_bias_ref.py on 256 of the walks, which the device's paths must equal), and the CA-GrQc accuracy of
default knobs at the three settings.  With a third argument "epoch" also the wall time of one default-knob pre-training
epoch on the bench graph (2.2e10 rows, 5.4e6 optimizer steps: minutes)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import graphgan_amd as ga  # noqa: E402
from graphgan_amd import pretrain, workloads  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
S = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
WPS, LEN, WINDOW, NEG, BATCH = 10, 40, 5, 5, 4096
COPY_CEILING = 6.29e12

rowptr, col, emb, n_edges = workloads.powerlaw_workload(n, n_emb=128)
eng = ga.Engine(emb, emb, lr_dis=5e-3, optimizer=ga.GG_OPT_ADAM_LAZY)
eng.set_graph_csr(rowptr, col)
eng.pretrain_set_noise(pretrain.noise_weights(rowptr))
starts = np.random.RandomState(5).choice(n, S, replace=False).astype(np.int32)
eng.prepare_pretrain(starts, WPS, LEN, WINDOW, NEG, 1, 0)  # warm-up: code objects, buffers
wall, walk_ms, fill_ms, rows = [], [], [], 0
for rep in range(3):
    c0 = eng.counters()
    t = time.perf_counter()
    rows = eng.prepare_pretrain(starts, WPS, LEN, WINDOW, NEG, 1, 1 + rep)
    wall.append(time.perf_counter() - t)
    c1 = eng.counters()
    walk_ms.append(c1["walk_kernel_ms"] - c0["walk_kernel_ms"])
    fill_ms.append(c1["last_kernel_ms"])
# the node2vec leg: the same starts, the walk kernel of P2b (the first call of a setting also sorts the lists: warm-up)
biased = {}
for p_, q_ in ((0.25, 4.0), (4.0, 0.25)):
    bias = pretrain.walk_bias(p_, q_)
    eng.pretrain_set_walk_bias(*bias)
    eng.prepare_pretrain(starts, WPS, LEN, WINDOW, NEG, 1, 0)
    b_walk, b_fill = [], []
    for rep in range(3):
        c0 = eng.counters()
        b_rows, b_paths, b_len = eng.prepare_pretrain(starts, WPS, LEN, WINDOW, NEG, 1, 1 + rep, fetch=True)
        c1 = eng.counters()
        b_walk.append(c1["walk_kernel_ms"] - c0["walk_kernel_ms"])
        b_fill.append(c1["last_kernel_ms"])
    from tests.support import pretrain_bias_ref as bref
    sub, st = np.sort(np.random.RandomState(6).choice(S, 256 // 4, replace=False)), {}
    o_paths, o_len = bref.walks(rowptr, col, starts[sub], 4, LEN, 1, 3, bias, stats=st)  # walks w = 0 .. 3 of 64 starts, stream of the last rep
    pick = (sub[:, None] * WPS + np.arange(4)[None, :]).reshape(-1)
    assert np.array_equal(b_paths[pick], o_paths) and np.array_equal(b_len[pick], o_len)
    biased["p%g_q%g" % (p_, q_)] = dict(
        weights=list(bias), walk_kernel_ms=min(b_walk), walk_kernel_ms_runs=[round(x, 4) for x in b_walk], fill_kernel_ms=min(b_fill),
        rows=int(b_rows), walk_over_uniform_walk=min(b_walk) / min(walk_ms), walk_over_fill=min(b_walk) / min(b_fill),
        oracle_walks=256, oracle_biased_hops=int(st["biased_hops"]), oracle_fallback_hops=int(st["fallback_hops"]),
        fallback_share_of_biased_hops=st["fallback_hops"] / max(1, st["biased_hops"]))
eng.pretrain_set_walk_bias(1, 1, 1)
eng.prepare_pretrain(starts, WPS, LEN, WINDOW, NEG, 1, 3)  # the uniform rows of the last repetition again, for the pass below
# byte model of the fill kernel: 12 B written per row; per walk its path (4 B per node), length and two row offsets; per
# negative the global levels of the prefix-sum search (log2 of the block the LDS subsample leaves) at 64-byte sectors
walks = S * WPS
levels = int(np.ceil(np.log2(max(2, -(-n // 2048)))))
neg_rows = rows // (1 + NEG) * NEG
model = dict(row_bytes=12 * rows, path_bytes=walks * (4 * LEN + 4 + 16), search_bytes=neg_rows * levels * 64)
model_total = sum(model.values())
# one fused discriminator pass over the same rows: the consumer the producer feeds
pass_starts = np.arange(0, rows, BATCH, dtype=np.int64)
np.random.RandomState(1).shuffle(pass_starts)
t = time.perf_counter()
eng.d_pass(pass_starts, BATCH)
eng.synchronize()
d_pass_s = time.perf_counter() - t
eng.close()
out = dict(n_node=n, n_edges=int(n_edges), n_emb=128, starts=S, walks_per_start=WPS, walk_len=LEN, window=WINDOW, n_neg=NEG, rows=int(rows),
           prepare_wall_ms=[round(x * 1e3, 3) for x in wall], rows_per_s=rows / min(wall), walk_kernel_ms=min(walk_ms),
           walk_kernel_ms_runs=[round(x, 4) for x in walk_ms], fill_kernel_ms=min(fill_ms), biased=biased,
           fill_byte_model=model, fill_model_bytes_per_s=model_total / (min(fill_ms) * 1e-3), fill_fraction_of_copy_ceiling=model_total / (min(fill_ms) * 1e-3) / COPY_CEILING,
           search_levels_global=levels, d_pass_batch=BATCH, d_pass_ms=d_pass_s * 1e3, prepare_over_d_pass=min(wall) / d_pass_s)
if len(sys.argv) > 3 and sys.argv[3] == "epoch":
    t = time.perf_counter()
    pretrain.pretrain(type("C", (), dict(n_emb=128))(), n, rowptr, col)
    out["default_epoch_wall_s"] = time.perf_counter() - t
if True:
    from tests.helpers import load_ca_grqc
    from oracle import graphgan_oracle as orc
    d, nc, _ = load_ca_grqc()
    rp, cl = ga.edges_to_csr(nc, d["train"])
    for key, (p_, q_) in (("ca_grqc_default_knobs_accuracy", (1.0, 1.0)), ("ca_grqc_default_knobs_accuracy_p0.25_q4", (0.25, 4.0)),
                          ("ca_grqc_default_knobs_accuracy_p4_q0.25", (4.0, 0.25))):
        table = pretrain.pretrain(type("C", (), dict(engine_seed=1, engine_pretrain_p=p_, engine_pretrain_q=q_))(), nc, rp, cl)
        out[key] = orc.eval_link_prediction(table.astype(np.float64), d["test"].tolist(), d["test_neg"].tolist())
print(json.dumps(out))
