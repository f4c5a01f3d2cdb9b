#!/usr/bin/env python3
"""The generator's exact graph softmax (gg_graph_softmax) on the bench graph and on CA-GrQc.
    python tools/graph_softmax_bench.py [n_node] [n_roots]        (default 10^6 1024)
Setup: the power-law bench graph (m = 10: ~10^7 edges, d = 128), whole trees of n_roots roots built on the device, G-mode.
One JSON line: the sweep's kernel time per root (best of 3; the queried path, one node per root, so no n_roots x N download),
the edge-score fill (wall time of a call right after the generator changed minus the same call on valid scores, median of 3),
the byte model of the sweep and its fraction of 8 TB/s, and all 5 242 CA-GrQc roots as a second leg."""
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
R = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
HBM = 8.0e12


def sweep(eng, slots, reps=3):
    q = [np.array([0], np.int32)] * len(slots)
    best, wall = None, None
    for _ in range(reps):
        t = time.time()
        eng.graph_softmax(slots, nodes=q)
        wall = time.time() - t
        best = eng.last_graph_softmax_ms if best is None else min(best, eng.last_graph_softmax_ms)
    return best, wall


def fill_ms(eng, bias):
    """wall of a one-slot call right after the generator changed minus the same call on valid scores"""
    d = []
    for _ in range(3):
        eng.set_bias(0, bias)  # (a table upload: the private edge scores are stale)
        t = time.time()
        eng.graph_softmax([0], nodes=[np.array([0], np.int32)])
        cold = time.time() - t
        t = time.time()
        eng.graph_softmax([0], nodes=[np.array([0], np.int32)])
        d.append((cold - (time.time() - t)) * 1e3)
    return float(np.median(d))


def byte_model(nodes):
    """bytes of the sweep per rank: streamed -- cstart (4), t_edge (4), t_order (4), logR written by the parent and read (8 + 8),
    the dense row's -inf fill (4 per node of the row); random -- the child's score, the father's reverse edge and score, the
    dense scatter: 4 gathers at 64-byte sectors"""
    streamed = 4 + 4 + 4 + 8 + 8 + 4
    random = 4 * 64
    return streamed + random, nodes * (streamed + random)


t0 = time.time()
rowptr, col, emb, n_edges = workloads.powerlaw_workload(n, n_emb=128)
t_gen = time.time() - t0
eng = ga.Engine(emb, emb, optimizer=ga.GG_OPT_SGD)
eng.set_graph_csr(rowptr, col)
bias = np.random.default_rng(6).normal(0, 0.3, n).astype(np.float32)
eng.set_bias(0, bias)
deg = rowptr[1:] - rowptr[:-1]
roots = np.sort(np.random.default_rng(7).choice(np.flatnonzero(deg > 0), R, replace=False)).astype(np.int32)
eng.set_tree_mode(0)
t = time.time()
eng.build_trees(roots, device=True)
t_bfs = time.time() - t
nodes = float(eng.tree_entries + R) / 2.0  # sum of C_r (2 C_r - 1 entries per root)
slots = np.arange(R, dtype=np.int32)
f_ms = fill_ms(eng, bias)
ms, wall = sweep(eng, slots)
per_rank, total = byte_model(nodes)
out = {"workload": "graph softmax, G-mode: %d whole trees of a %d-node power-law graph (%d edges), n_emb=128" % (R, n, n_edges),
       "workload_gen_s": t_gen, "bfs_s": t_bfs, "tree_nodes": nodes,
       "es_fill_ms": f_ms, "es_fill_target_ms": 3.0,
       "sweep_kernel_ms": ms, "sweep_call_s": wall, "us_per_root": ms * 1e3 / R, "us_per_root_target": 100.0,
       "bytes_per_rank_model": per_rank, "bytes_model": total, "achieved_TBps": total / (ms * 1e-3) / 1e12,
       "frac_of_8TBps": total / (ms * 1e-3) / HBM}
eng.close()

# second leg: all CA-GrQc roots (whole trees, pre-trained rows + random bias)
from tests.helpers import ca_grqc_init_embeddings, load_ca_grqc  # noqa: E402
d, nc, _ = load_ca_grqc()
embc = ca_grqc_init_embeddings(d, nc).astype(np.float32)
rp, cl = ga.edges_to_csr(nc, d["train"])
eng = ga.Engine(embc, embc)
eng.set_graph_csr(rp, cl)
eng.set_bias(0, np.random.default_rng(8).normal(0, 0.5, nc).astype(np.float32))
eng.set_tree_mode(0)
eng.build_trees(np.arange(nc, dtype=np.int32), device=True)
cf_ms = fill_ms(eng, eng.get_bias(0))
cms, cwall = sweep(eng, np.arange(nc, dtype=np.int32))
out["ca_grqc"] = {"roots": nc, "sweep_kernel_ms": cms, "sweep_call_s": cwall, "es_fill_ms": cf_ms, "target_ms": 50.0}
eng.close()
print(json.dumps(out))
