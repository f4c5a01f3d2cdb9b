#!/usr/bin/env python3
"""The pair-neighbour sweep (gg_pair_neighbors) on the synthetic power-law workload: the neighbourhood link-prediction indices
of 10^6 training edges and of 10^6 uniform random pairs, as separate legs (a training edge of a power-law graph very often has a
hub at one end; a random pair rarely has), with the two fixed-point weight arrays of Adamic-Adar and resource allocation.
    python tools/pair_neighbors_bench.py [n_node] [n_emb] [n_pairs]        (default 10^6 128 10^6)
One JSON line.  Per leg: kernel_ms (best of 3, the legs alternating) and call_s of Engine.pair_neighbors, pairs/s and entries of
the shorter lists probed/s, the share of pairs split into chunk tasks, a byte model (the shorter list read once, 4 B an entry,
plus one 8 B weight per common neighbour and weight array: what the sweep cannot avoid reading; the searched list's probes are
not counted) and its GB/s; beside it, in the same run, the embedding side's cost of scoring the same pairs --
gg_edge_classifier_predict's call_s (it reports no device time) and the device ms of one gg_edge_classifier_fit sweep over
them -- and a SINGLE-THREAD numpy intersection (link_heuristics.host_pair_neighbors) on a 10^4-pair sample of each leg, whose
integers must equal the device's.  Nothing is gated."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import graphgan_amd as ga  # noqa: E402
from graphgan_amd import workloads  # noqa: E402
from graphgan_amd.evaluation import link_heuristics as lh  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 128
m = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
SAMPLE = 10_000
t0 = time.time()
rowptr, col, emb, n_edges = workloads.powerlaw_workload(n, n_emb=d)
t_gen = time.time() - t0
eng = ga.Engine(emb, emb, optimizer=ga.GG_OPT_SGD)  # SGD: no Adam slots
eng.set_graph_csr(rowptr, col)
rs = np.random.default_rng(7)
pos = rs.integers(0, len(col), m)  # a training edge = an adjacency entry drawn uniformly
legs = {"train_edges": ((np.searchsorted(rowptr, pos, side="right") - 1).astype(np.int32), col[pos].astype(np.int32)),
        "random_pairs": (rs.integers(0, n, m).astype(np.int32), rs.integers(0, n, m).astype(np.int32))}
t0 = time.time()
deg = eng.distinct_degrees()  # (builds the set adjacency: host sort + upload, once per graph)
t_adj = time.time() - t0
w = lh.node_weights(deg)
chunk = ga.Engine.PAIR_NEIGHBORS_CHUNK
out = {"workload": "pair-neighbour sweep: %d pairs per leg on the power-law graph of %d nodes / %d edges, n_w = 2 (aa, ra); embedding side: n_emb=%d"
                   % (m, n, n_edges, d), "workload_gen_s": t_gen, "set_adjacency_s": t_adj, "max_distinct_degree": int(deg.max()),
       "mean_distinct_degree": float(deg.mean()), "chunk": chunk, "untuned": "group widths 4 / 16 / 64, chunk and grid are the first shape built"}

best = dict((k, None) for k in legs)
wall, last = {}, {}
for _ in range(3):  # alternating, so that both legs see the same clocks
    for name, (u, v) in legs.items():
        t = time.time()
        res = eng.pair_neighbors(u, v, w)
        wall[name] = time.time() - t
        best[name] = res["kernel_ms"] if best[name] is None else min(best[name], res["kernel_ms"])
        last[name] = res

wz, bz = (rs.standard_normal(d) * 0.1).astype(np.float32), 0.0
ptr_h = adj_h = None
for name, (u, v) in legs.items():
    res, ms = last[name], best[name]
    short = np.minimum(res["deg_u"], res["deg_v"]).astype(np.int64)
    probed, cn = int(short.sum()), int(res["cn"].astype(np.int64).sum())
    model = 4.0 * probed + 8.0 * 2 * cn
    leg = {"kernel_ms": ms, "call_s": wall[name], "pairs_per_s": m / (ms * 1e-3), "entries_probed": probed, "entries_probed_per_s": probed / (ms * 1e-3),
           "common_neighbours": cn, "mean_shorter_list": float(short.mean()), "max_shorter_list": int(short.max()),
           "chunked_share": float((short > chunk).mean()), "width_share": [float((short <= 8).mean()), float(((short > 8) & (short <= 64)).mean()),
                                                                           float((short > 64).mean())],
           "model_bytes": model, "model_GBps": model / (ms * 1e-3) / 1e9}
    # the embedding side on the same pairs
    eng.edge_classifier_predict(u, v, wz, bz)
    t = time.time()
    eng.edge_classifier_predict(u, v, wz, bz)
    leg["edge_classifier_predict_call_s"] = time.time() - t
    leg["edge_classifier_sweep_ms"] = eng.edge_classifier_fit(u, v, (np.arange(m) & 1).astype(np.int32), iters=1)["ms"]
    leg["sweep_over_edge_classifier_sweep"] = ms / leg["edge_classifier_sweep_ms"]
    # single-thread numpy on a sample; its integers are the device's
    if ptr_h is None:
        ptr_h, adj_h = lh.csr_set_adjacency(rowptr, col)
    su, sv = u[:SAMPLE], v[:SAMPLE]
    t = time.time()
    host = lh.host_pair_neighbors(ptr_h, adj_h, su, sv, w)
    t_host = time.time() - t
    leg["host_numpy_single_thread"] = {"pairs": len(su), "s": t_host, "pairs_per_s": len(su) / t_host,
                                       "device_over_host_pairs_per_s": leg["pairs_per_s"] / (len(su) / t_host)}
    leg["host_sample_equal"] = bool(all(np.array_equal(host[k], res[k][..., :SAMPLE]) for k in ("cn", "deg_u", "deg_v", "wsum")))
    out[name] = leg
eng.close()
print(json.dumps(out))
