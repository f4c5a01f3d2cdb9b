#!/usr/bin/env python3
"""bench.py -- the GraphGAN hot path on MI355X, one JSON line.

Metric (BASELINE.json): sampled-edges/sec of the graph-softmax walk sampler, with the D-step /
G-step pairs/sec beside it.  One *step* = one epoch body of the reference's ``train()``
(src/GraphGAN/graph_gan.py:144-176 with one inner pass each) over this rank's R root slots:

    prepare_data_for_d (D-mode walks, deg(root) each)  ->  one D optimizer pass over those rows
    prepare_data_for_g (G-mode walks, n_sample_gen=20, window pairs, rewards) -> one G pass

``value`` = sampled edges (hops of both walk launches, all ranks) / wall time of the K timed
steps, inputs resident in HBM.  Workload at N=1: synthetic power-law graph, 1M nodes / 10M
edges, n_emb = 128 (the configuration the north-star target is quoted on), R = 16 384 roots per step
(197 GB of resident trees; the 8 192-root batch of rounds 1-2 is reported beside it).
Weak scaling: every rank walks its own R roots; replicas exchange gradients through RCCL.

    python bench.py [--gpus N --steps K --warmup W]              (N > 1: spawns its own N ranks, one per GPU)
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...   (the driver's launcher: same ranks)

A plain run sets up, warms up, times the K steps and prints the line (with the figures derived from the timed region's
own counters and events).  ``--full`` adds every leg behind the timed region: the 8 192-root continuity batch, the solo
kernel events, the fresh-batch end-to-end figures, the strict-mode lines and the CPU baselines.  ``--dump-outputs DIR``
writes what the last timed step computed (sampled rows of both tables and biases, sampled prepared D rows and G pairs)
as DIR/<name>.npy, so that two builds can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s spec, ~6.3 TB/s achievable)


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--workload", default="powerlaw", choices=["powerlaw", "ca_grqc"])
    p.add_argument("--nodes", type=int, default=1_000_000)
    p.add_argument("--m", type=int, default=10)
    p.add_argument("--emb", type=int, default=128)
    p.add_argument("--roots", type=int, default=16384, help="root slots per rank per step (16 384 trees of the 1M-node graph = 197 GB of the 288 GB HBM; "
                                                                "rounds 1-2 ran 8 192: that batch is reported beside it as `batch_of_rounds_1_2`)")
    p.add_argument("--continuity-roots", type=int, default=8192, help="behind the timed region: the same steps over this many of the resident roots (0 = skip)")
    p.add_argument("--n-sample-gen", type=int, default=20)
    p.add_argument("--optimizer", default="adam_lazy", choices=["adam_dense", "adam_lazy", "sgd"])
    p.add_argument("--threads", type=int, default=0, help="host BFS threads (0 = min(64, cores))")
    p.add_argument("--host-bfs", action="store_true", help="build the BFS trees on host threads instead of on the GPU")
    p.add_argument("--cpu-baseline-seconds", type=float, default=15.0)
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--seed", type=int, default=6)
    p.add_argument("--no-g-head-start", action="store_true", help="do not call gg_prepare_g_begin before the D pass (the G-mode walks then start once the host has enqueued the D pass)")
    p.add_argument("--overlap-steps", type=int, default=6, help="steps behind the timed region whose profiled side-stream launches ARE isolated (solo roofline figure)")
    p.add_argument("--fresh-batches", type=int, default=2, help="behind the timed region: root batches whose trees are built first (end-to-end figure); 0 = skip")
    p.add_argument("--no-strict", action="store_true", help="skip the strict-mode (batch 64, dense TF1-Adam, CA-GrQc) pairs/s line")
    p.add_argument("--profile-every", type=int, default=3,
                   help="HIP events around every k-th walk launch of the timed region (an event pair costs ~6 us of stream bubble on "
                        "each side of every level_score_kernel launch; an odd k alternates between the D-mode and G-mode launches)")
    p.add_argument("--full", action="store_true", help="also run every leg behind the timed region (continuity batch, solo kernel events, "
                                                       "fresh batches, strict mode, CPU baselines); a plain run only times the steps")
    p.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed as DIR/<name>.npy (fixed, seeded samples)")
    return p.parse_args()


def make_workload(args, ga):
    if args.workload == "ca_grqc":
        g = np.load(os.path.join(ROOT, "tests", "golden", "ca_grqc.npz"))
        n = int(g["n_node"])
        rowptr, col = ga.edges_to_csr(n, g["train"])
        emb = np.random.RandomState(5).rand(n, g["emb_rows"].shape[1])
        emb[g["emb_ids"]] = g["emb_rows"]
        name = "CA-GrQc (5242 nodes, 13046 train edges), n_emb=50, shipped pre-trained embeddings"
        return n, rowptr, col, emb.astype(np.float32), name
    from graphgan_amd import workloads
    n, d = args.nodes, args.emb
    rowptr, col, emb, n_edges = workloads.powerlaw_workload(n, args.m, d)  # SURVEY.md section 8d recipe (also what tests/test_gpu_scale.py checks)
    name = "synthetic power-law (Barabasi-Albert m=%d): %d nodes / %d edges, n_emb=%d" % (args.m, n, n_edges, d)
    return n, rowptr, col, emb, name


def cpu_baseline(args, n, rowptr, col, emb, bias, roots, seconds):
    """The C oracle ('port' of graph_gan.py:225-270 with scores computed on demand, i.e. the
    'hoisted' fair baseline of BASELINE.md section 3) on ONE host core, G-mode walks over a bounded
    sample of this workload's roots; returns (edges/s, sample description)."""
    from oracle import graphgan_oracle as orc
    Ep = orc.pad_rows(emb)
    # a representative sample: evenly spaced through the degree-sorted root list (not just the hub roots)
    rts = np.ascontiguousarray(roots[:: max(1, len(roots) // 48)][:48])
    # trees are a cached precompute in the reference too (graph_gan.py:31-46): not timed
    off, nbr, base, dmax = orc.c_build_trees(n, rowptr, col, rts)
    slots = np.arange(len(rts), dtype=np.int32)
    nw = np.full(len(rts), args.n_sample_gen, dtype=np.int32)
    hops, t, stream = 0, 0.0, 1
    while t < seconds:
        t0 = time.perf_counter()
        res = orc.c_walk_sample(Ep, bias, off, nbr, base, rts, slots, nw, False, args.seed, stream, dmax + 3)
        t += time.perf_counter() - t0
        hops += int(res["hops"])
        stream += 2
    return hops / t, "G-mode walks (%d per root) from %d roots of the same graph, repeated over %d RNG streams: %d hops in %.1f s, scores computed on demand (hoisted flavour)" % (
        args.n_sample_gen, len(rts), stream // 2, hops, t)


def cpu_baseline_threads(args, n, rowptr, col, emb, bias, roots, seconds, threads):
    """The same C port on MANY host cores: `threads` Python threads, each with four roots of its own (trees built by the thread,
    not timed), each calling the C walk sampler in a loop until the deadline -- ctypes releases the GIL inside the call, the
    library keeps no state, G-mode walks only read the trees.  Whole-host rate = hops of all threads / wall time.  No fork and no
    subprocess: the HIP runtime is live in this process."""
    import threading
    from oracle import graphgan_oracle as orc
    Ep = orc.pad_rows(emb)
    per = 4
    pick = np.ascontiguousarray(roots[:: max(1, len(roots) // (threads * per))][: threads * per])
    threads = max(1, len(pick) // per)
    state = [None] * threads
    ready = threading.Barrier(threads + 1)
    hops = [0] * threads
    err = []
    deadline = [0.0]

    def work(i):
        try:
            rts = np.ascontiguousarray(pick[i * per:(i + 1) * per])
            off, nbr, base, dmax = orc.c_build_trees(n, rowptr, col, rts)
            slots = np.arange(len(rts), dtype=np.int32)
            nw = np.full(len(rts), args.n_sample_gen, dtype=np.int32)
            state[i] = True
        except Exception as e:  # noqa: BLE001  (reported, never fatal for the bench line)
            err.append(repr(e))
            state[i] = False
        ready.wait()
        ready.wait()  # the main thread has set the deadline
        if not state[i]:
            return
        stream = 1 + 2 * i
        while time.perf_counter() < deadline[0]:
            res = orc.c_walk_sample(Ep, bias, off, nbr, base, rts, slots, nw, False, args.seed, stream, dmax + 3)
            hops[i] += int(res["hops"])
            stream += 2 * threads

    ts = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(threads)]
    for t in ts:
        t.start()
    ready.wait()
    t0 = time.perf_counter()
    deadline[0] = t0 + seconds
    ready.wait()
    for t in ts:
        t.join(timeout=seconds + 60)
    dt = time.perf_counter() - t0
    if err:
        return {"error": err[0]}
    return {"value": sum(hops) / dt, "unit": "edges/s", "cores": threads, "host_cores_on_box": os.cpu_count(), "kind": "port",
            "sample": "G-mode walks (%d per root) from %d roots (%d per thread) of the same graph, every thread looping over RNG streams for %.1f s: %d hops"
                      % (args.n_sample_gen, threads * per, per, dt, sum(hops))}


def cpu_baseline_faithful(n_roots=24):
    """The 'faithful' flavour of SURVEY.md section 8d on BASELINE configs[0..1] (CA-GrQc, n_emb = 50): like the reference,
    EVERY sample() call first recomputes the full N x N score matrix (graph_gan.py:238, generator.py:21: E.E^T + b, numpy on
    the host's BLAS threads) and then walks (C oracle, one core).  Timed on a bounded sample of roots; the N x N matrix
    cannot exist for the 1M-node workload, so this flavour is only reported here."""
    from oracle import graphgan_oracle as orc
    g = np.load(os.path.join(ROOT, "tests", "golden", "ca_grqc.npz"))
    n = int(g["n_node"])
    import graphgan_amd as ga
    rowptr, col = ga.edges_to_csr(n, g["train"])
    emb = np.random.RandomState(5).rand(n, g["emb_rows"].shape[1])
    emb[g["emb_ids"]] = g["emb_rows"]
    emb = emb.astype(np.float32)
    bias = np.zeros(n, np.float32)
    deg = rowptr[1:] - rowptr[:-1]
    roots = np.flatnonzero(deg > 0)[:: max(1, int((deg > 0).sum()) // n_roots)][:n_roots].astype(np.int32)
    off, nbr, base, dmax = orc.c_build_trees(n, rowptr, col, roots)
    Ep = orc.pad_rows(emb)
    t_mm = 0.0
    for _ in roots:  # one all_score per sample() call
        t0 = time.perf_counter()
        S = emb @ emb.T + bias[None, :]
        t_mm += time.perf_counter() - t0
    assert S.shape == (n, n)
    t0 = time.perf_counter()
    res = orc.c_walk_sample(Ep, bias, off, nbr, base, roots, np.arange(len(roots), dtype=np.int32), np.full(len(roots), 20, np.int32), False, 6, 1, dmax + 3)
    t_walk = time.perf_counter() - t0
    hops = int(res["hops"])
    return {"value": hops / (t_mm + t_walk), "unit": "edges/s", "kind": "port", "flavour": "faithful: all_score (N x N) recomputed per sample() call",
            "cores": os.cpu_count(), "workload": "CA-GrQc (5242 nodes), n_emb=50, G-mode walks (20 per root)",
            "sample": "%d roots: %d hops, %.2f s in %d matmuls of %.0f MFLOP (numpy BLAS threads), %.3f s walking (one core)" % (
                len(roots), hops, t_mm, len(roots), 2e-6 * n * n * emb.shape[1], t_walk)}


def pmc_traffic(kernel_substr):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC summary
    (profiles/summarize.py; FETCH_SIZE / WRITE_SIZE collected in separate passes of this same
    command, gfx950 correction applied).  PMC counters cannot be read from inside the bench."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_hbm_traffic.json")))
    if not files:
        return None, None
    data = json.load(open(files[-1]))
    for name, v in data.items():
        if kernel_substr in name and not name.startswith("_"):
            return v["hbm_bytes_per_launch"], os.path.relpath(files[-1], ROOT)
    return None, None


def pmc_same_run():
    """Algorithmic bytes per launch of the dominant kernel as counted by the bench run the PMC pass itself profiled
    (profiles/summarize.py stores that run's own bench line next to its traffic): traffic / algorithmic inside ONE run."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_hbm_traffic.json")))
    if not files:
        return None
    return json.load(open(files[-1])).get("_same_run")


def delta(c1, c0):
    return {k: c1[k] - c0[k] for k in c1}


DUMP_TABLE_BYTES = 16 << 20  # rows of each embedding table sampled so that one table's sample is at most 16 MB ...
DUMP_TABLE_ROWS = 1 << 16    # ... and at most this many rows (the bias samples: narrow tables)
DUMP_PAIRS = 1 << 18         # prepared D rows / G pairs sampled


def dump_outputs(eng, out_dir):
    """What the last timed step computed, as a caller of the step receives it: both models' embeddings and biases after its
    D and G passes, the D rows (center, neighbor, label) and the G pairs (node_1, node_2, reward) it prepared.  Fixed, seeded
    samples (the same rows for the same arguments); values float32, node ids float64; well under 64 MB in all."""
    os.makedirs(out_dir, exist_ok=True)
    n, d = eng.n_node, eng.n_emb
    rows = np.sort(np.random.RandomState(0).choice(n, min(n, DUMP_TABLE_ROWS, max(1, DUMP_TABLE_BYTES // (4 * d))), replace=False))
    arrays = {}
    for which, name in ((0, "gen"), (1, "dis")):
        arrays[name + "_emb_rows"] = eng.get_embeddings(which)[rows]
        arrays[name + "_bias_rows"] = eng.get_bias(which)[rows]

    def sample(k):
        return np.sort(np.random.RandomState(1).choice(k, DUMP_PAIRS, replace=False)) if k > DUMP_PAIRS else np.arange(k)
    c, nb, lab = eng.get_d_data()
    i = sample(len(c))
    arrays.update(d_center=c[i].astype(np.float64), d_neighbor=nb[i].astype(np.float64), d_label=lab[i])
    a, b, r = eng.get_g_data()
    i = sample(len(a))
    arrays.update(g_node_1=a[i].astype(np.float64), g_node_2=b[i].astype(np.float64), g_reward=r[i])
    assert sum(v.nbytes for v in arrays.values()) <= 64 << 20
    for name, v in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), v)


def exchange_label(comm):
    """What the replicas' gradient exchanges of this run actually were (gg_comm_stats), not what was planned."""
    if not comm:
        return "none (counters unavailable)"
    pk, ow, de = comm.get("pack_steps", 0), comm.get("owner_steps", 0), comm.get("dense_steps", 0)
    kinds = []
    if pk:
        kinds.append("%d x all-gather of fixed-capacity row packs" % pk)
    if ow:
        kinds.append("%d x owner-partitioned send / recv + all-gather of the reduced rows (%s rows)" % (ow, "bf16" if comm.get("bf16_rows") else "fp32"))
    if de:
        kinds.append("%d x dense reduce-scatter + all-gather of the accumulators" % de)
    return ", ".join(kinds) if kinds else "no exchange ran"


N_CU = 256                # MI355X: 8 XCDs x 32 compute units
ENGINE_CLOCK_HZ = 2.4e9   # peak engine clock
XGMI_LINK_GBS = 153.0   # per direction and link; 7 links per GPU, point to point (the task brief's figure: the guides give none)
XGMI_EFFICIENCY = 0.8   # assumed payload fraction of the link rate for RCCL send / recv of >= 1 MB segments (NOT measured)
HOST_ROUND_TRIP_MS = 0.03  # the owner exchange's two small host synchronisations (count matrix, largest owner), each


def comm_model(n, ld, d_rows_touched, g_rows_touched, d_pairs, g_pairs, step_ms=None, d_pass_ms=None, g_walk_ms=None, epoch=None):
    """Bytes ONE rank sends per step (D exchange + G exchange) at P = 2 / 4 / 8 under each strategy, from this run's real
    per-rank counts (touched rows of the two passes, pairs of the two passes).  Weak scaling: every rank brings the same
    counts.  dense = reduce-scatter + all-gather of the [N, ld + 1] accumulators (+ the int32 row flags);
    packs = all-gather of fixed-capacity row packs, capacity min(N, 2 * pairs) rows of (ld + 2) words, sent to P - 1 peers;
    owner = owner-partitioned sparse reduce: each touched row goes to its owner (row mod P), the owner's reduced rows -- the
    union over ranks, bounded by min(N, P * touched) -- go to the P - 1 peers; owner_bf16 = the same with bf16 rows
    (GG_COMM_BF16=1).  TIME (round 5): every transfer of the owner exchange is a personalised all-to-all / all-gather in which
    each pair of ranks uses its own xGMI link, so a rank's bytes move over P - 1 links at once: ms = bytes / ((P - 1) x link
    rate x efficiency) + two host round trips.  EXPOSED time per step: the D exchange runs on the main stream beside the G-mode
    walks of the side stream (gg_prepare_g_begin), so only what (D pass + D exchange) exceeds those walks by is exposed; the G
    exchange sits between the generator's gradient and optimizer kernels with nothing to hide behind (the next D-mode walks
    need the updated generator).  Estimated weak-scaling efficiency = step / (step + exposed).  No N > 1 run exists: a MODEL."""
    row_b = 4.0 * (ld + 2)
    row_h = 2.0 * (ld + 2) + 4.0
    out = {}
    for P in (2, 4, 8):
        f = (P - 1.0) / P
        dense = 2 * (2.0 * f * 4.0 * n * (ld + 1) + 2.0 * f * 4.0 * n)
        packs = sum((P - 1) * min(n, 2 * pairs) * row_b for pairs in (d_pairs, g_pairs))
        own = {"fp32": [f * t * row_b + f * min(n, P * t) * row_b for t in (d_rows_touched, g_rows_touched)],
               "bf16": [f * t * row_h + f * min(n, P * t) * row_h for t in (d_rows_touched, g_rows_touched)]}
        entry = {"dense_rs_ag": dense, "row_packs_allgather": packs, "owner_partitioned_sparse": sum(own["fp32"]),
                 "owner_partitioned_sparse_bf16": sum(own["bf16"]),
                 # (steps.hip::exchange_sparse: packs while world x capacity < 1.5 N rows; above that the owner-partitioned
                 # exchange when the bound is >= GG_COMM_OWNER_MIN rows and ncclSend / ncclRecv resolve, else dense)
                 "picked_today": ("row_packs_allgather" if P * min(n, 2 * max(d_pairs, g_pairs)) < 1.5 * n else
                                  "owner_partitioned_sparse (dense_rs_ag if ncclSend / ncclRecv are missing or GG_COMM_OWNER=0)")}
        rate = (P - 1) * XGMI_LINK_GBS * 1e9 * XGMI_EFFICIENCY  # bytes / s leaving one rank over the links the exchange uses
        for kind, (bd, bg) in own.items():
            d_ms, g_ms = 1e3 * bd / rate + 2 * HOST_ROUND_TRIP_MS, 1e3 * bg / rate + 2 * HOST_ROUND_TRIP_MS
            t = {"d_exchange_ms": d_ms, "g_exchange_ms": g_ms}
            if step_ms and d_pass_ms is not None and g_walk_ms is not None:
                exposed = max(0.0, d_pass_ms + d_ms - g_walk_ms) + g_ms
                t.update(exposed_ms_per_step=exposed, weak_scaling_efficiency_estimate=step_ms / (step_ms + exposed))
            entry["modelled_time_owner_%s" % kind] = t
        entry["modelled_time_dense_ms"] = 1e3 * dense / rate
        out["P=%d" % P] = entry
    out["assumptions"] = {"xgmi_link_GBs": XGMI_LINK_GBS, "links_used": "P - 1 (one per peer)", "link_efficiency": XGMI_EFFICIENCY,
                          "host_round_trip_ms": HOST_ROUND_TRIP_MS, "step_ms": step_ms, "d_pass_ms": d_pass_ms, "g_walk_ms": g_walk_ms}
    if epoch:
        # The OTHER metric that scales: one outer epoch of GraphGAN.train() over ALL roots (root batches, gg_epoch_*): its prepare
        # phase -- tree build, D- and G-mode walks of every root batch -- has NO collective (roots are sharded, the walks' RNG is
        # keyed by the root), the inner passes exchange once per optimizer step over fused batches of 2^22 rows (dense: at that
        # size every row of the table is touched).  Strong scaling of a fixed epoch: T(P) = (prepare + passes) / P + steps x exchange.
        nb, prep, pas = epoch["n_batches"], epoch["prepare_s_per_batch"], epoch["pass_s_per_batch"]
        steps = -(-int(nb * d_pairs) // (1 << 22)) + -(-int(nb * g_pairs) // (1 << 22))
        t1 = nb * (prep + pas)
        ep = {"what": "MODELLED strong scaling of one outer epoch over all %d roots (%.0f root batches of this run's size): prepare phase "
                      "without any collective, %d optimizer steps with a dense exchange each" % (epoch["n_roots"], nb, steps),
              "one_gpu_s": t1, "prepare_share_one_gpu": nb * prep / t1}
        for P in (2, 4, 8):
            tp = t1 / P + steps * 1e-3 * out["P=%d" % P]["modelled_time_dense_ms"]
            ep["P=%d" % P] = {"epoch_s": tp, "strong_scaling_efficiency_estimate": t1 / (P * tp)}
        out["epoch_over_all_roots"] = ep
    return out


def strict_mode_line(ga, _lib, seconds=1.5):
    """SURVEY.md section 8d metric 2(i): the reference's own schedule -- batch 64, dense TF1-Adam over the whole table per
    step (graph_gan.py:149-157,168-176) -- on the CA-GrQc fixture (N = 5 242, d = 50), pairs/s through gg_d_pass /
    gg_g_pass over resident prepared data, wall clock around whole inner passes."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "ca_grqc.npz"))
    n = int(g["n_node"])
    rowptr, col = ga.edges_to_csr(n, g["train"])
    emb = np.random.RandomState(5).rand(n, g["emb_rows"].shape[1])
    emb[g["emb_ids"]] = g["emb_rows"]
    eng = ga.Engine(emb, emb, optimizer=_lib.GG_OPT_ADAM_DENSE)
    eng.set_graph_csr(rowptr, col)
    roots = np.arange(n, dtype=np.int32)
    eng.build_trees(roots, device=True)
    eng.set_profiling(0)
    out = {}
    rows = eng.prepare_d(roots, 1, 0, fetch=False)
    pairs = eng.prepare_g(roots, 20, 1, 1, fetch=False)
    rs = np.random.RandomState(0)
    for name, total, fn in (("d", rows, eng.d_pass), ("g", min(pairs, 64 * 6000), eng.g_pass)):
        starts = np.arange(0, total, 64, dtype=np.int64)
        fn(starts[:50], 64)
        eng.synchronize()
        done, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            rs.shuffle(starts)
            fn(starts, 64)
            eng.synchronize()
            done += len(starts)
        dt = time.perf_counter() - t0
        out["%s_pairs_per_sec" % name] = 64.0 * done / dt
        out["%s_us_per_step" % name] = 1e6 * dt / done
    out["config"] = "CA-GrQc (5242 nodes), n_emb=50, batch 64, dense TF1-Adam (24*N*(d+1) B per step), resident prepared data"
    eng.close()
    return out


def strict_mode_at_scale(ga, _lib, n, rowptr, col, emb, roots, n_sample_gen, seed, n_steps=3000):
    """SURVEY.md section 8d metric 2(i) on the BENCH graph: the reference's batching -- contiguous slices of 64 rows of the
    prepare-order lists in shuffled order, one optimizer step per slice (graph_gan.py:149-157,168-176) -- with the scale-mode
    optimizers (lazy Adam, SGD: a dense TF1-Adam sweep of a 1M x 128 table per 64 pairs is 1.5 GB of traffic per step and is
    what the fixture-sized line above prices), over the resident prepared rows of one step of `roots`, >= n_steps optimizer
    steps per model, wall clock around whole passes.  One launch per step: the atomic-free gradient kernel applies the
    optimizer itself (pair_grad_det_kernel, steps.hip)."""
    out = {}
    for name, opt in (("adam_lazy", _lib.GG_OPT_ADAM_LAZY), ("sgd", _lib.GG_OPT_SGD)):
        eng = ga.Engine(emb, emb, optimizer=opt)
        eng.set_graph_csr(rowptr, col)
        eng.build_trees(roots, device=True)
        eng.set_profiling(0)
        slots = np.arange(len(roots), dtype=np.int32)
        rows = eng.prepare_d(slots, seed, 0, fetch=False)
        pairs = eng.prepare_g(slots, n_sample_gen, seed, 1, fetch=False)
        rs = np.random.RandomState(0)
        line = {}
        for which, total, fn in (("d", rows, eng.d_pass), ("g", pairs, eng.g_pass)):
            starts = np.arange(0, total, 64, dtype=np.int64)
            rs.shuffle(starts)
            starts = starts[:n_steps]
            fn(starts[:50], 64)
            eng.synchronize()
            t0 = time.perf_counter()
            fn(starts, 64)
            eng.synchronize()
            dt = time.perf_counter() - t0
            line["%s_steps" % which] = int(len(starts))
            line["%s_pairs_per_sec" % which] = 64.0 * len(starts) / dt
            line["%s_us_per_step" % which] = 1e6 * dt / len(starts)
        out[name] = line
        eng.close()
    out["config"] = ("the bench graph (%d nodes), n_emb=%d, batch 64 (the reference's batching), lazy Adam / SGD, resident prepared rows of %d roots; "
                     "the headline d_step_pairs_per_sec / g_step_pairs_per_sec use ONE fused batch per pass instead" % (n, emb.shape[1], len(roots)))
    return out


def self_launch(n, script=None):
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves -- one process per GPU with the
    environment torch.distributed.run would export (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT; rendezvous
    on 127.0.0.1) -- pass rank 0's stdout (the JSON line) through, and fail if any rank fails."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), GG_BENCH_CHILD="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC (RCCL between processes of one node)
        env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or n) // n)))
        procs.append(subprocess.Popen([sys.executable, script or os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    out, _ = procs[0].communicate()
    rcs = [procs[0].returncode] + [p.wait() for p in procs[1:]]
    sys.stdout.write(out.decode())
    sys.stdout.flush()
    if any(rcs):
        raise SystemExit("bench.py --gpus %d: rank exit codes %s" % (n, rcs))


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return self_launch(args.gpus)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    share_gpu = os.environ.get("GG_BENCH_SHARE_GPU") == "1"  # plumbing test on a 1-GPU box: all ranks on device 0, no RCCL
    if share_gpu:
        local_rank = 0
    if world != args.gpus:  # started by a launcher with another --nproc-per-node: the launcher's world is what runs
        args.gpus = world

    import graphgan_amd as ga  # loads libgraphgan_hip.so (and with it the HIP runtime) before anything else
    from graphgan_amd import _lib

    from graphgan_amd import parallel
    ctl = parallel.Control(rank, world)  # control plane only (gloo on CPU): barrier, max, RCCL id broadcast

    t_setup = time.time()
    n, rowptr, col, emb, wl_name = make_workload(args, ga)
    opt = {"adam_dense": _lib.GG_OPT_ADAM_DENSE, "adam_lazy": _lib.GG_OPT_ADAM_LAZY, "sgd": _lib.GG_OPT_SGD}[args.optimizer]
    eng = ga.Engine(emb, emb, optimizer=opt, device=local_rank)
    eng.set_graph_csr(rowptr, col)
    from graphgan_amd import workloads
    roots = workloads.bench_roots(rowptr, args.roots, rank, world, args.seed)  # longest (hub) roots first
    R = len(roots)
    threads = args.threads or min(64, os.cpu_count() or 1)
    t_trees = time.time()
    if args.host_bfs:
        eng.build_trees(roots, n_threads=max(1, threads // max(1, min(world, 8))))
    else:
        eng.build_trees(roots, device=True)
    trees_s = time.time() - t_trees
    c_trees = eng.counters()
    slots = np.arange(len(roots), dtype=np.int32)
    if not share_gpu:
        ctl.connect_engine(eng)
        if world > 1:  # the replicas really are one RCCL communicator of N ranks
            assert eng.comm_stats()["world"] == world, "RCCL communicator has %d ranks, expected %d" % (eng.comm_stats()["world"], world)
    setup_s = time.time() - t_setup
    eng.set_profiling(args.profile_every)

    def step(i, head_start=True):
        # every rank issues both passes (they contain the replicas' gradient exchange), even with no rows
        rows = eng.prepare_d(slots, args.seed, 2 * i, fetch=False)
        if head_start and not args.no_g_head_start:  # the G-mode walks need the generator only: enqueued before the host enqueues the D pass
            eng.prepare_g_begin(slots, args.n_sample_gen, args.seed, 2 * i + 1)
        eng.d_pass(np.zeros(1, np.int64), max(int(rows), 1))
        pairs = eng.prepare_g(slots, args.n_sample_gen, args.seed, 2 * i + 1, fetch=False)
        eng.g_pass(np.zeros(1, np.int64), max(int(pairs), 1))

    def barrier():
        eng.comm_barrier()
        ctl.barrier()

    eng.set_profiling_solo(False)  # the timed region runs as production does: profiled G-mode walks stay beside the discriminator update
    for i in range(args.warmup):
        step(i)
    barrier()
    eng.set_profiling(args.profile_every)  # restart the cadence: the first launch of the timed region is a profiled one
    c0 = eng.counters()
    t0 = time.perf_counter()
    for i in range(args.warmup, args.warmup + args.steps):
        step(i)
    barrier()
    dt = time.perf_counter() - t0
    c1 = eng.counters()
    c = delta(c1, c0)
    comm = eng.comm_stats() if world > 1 and not share_gpu else None
    if args.dump_outputs and rank == 0:  # before any leg below changes the tables or the prepared data
        dump_outputs(eng, args.dump_outputs)

    # ---- behind the timed region, --full only (every rank takes part: the steps contain collectives) ------------
    nxt = args.warmup + args.steps
    # (0) continuity with rounds 1-2: the same step over the 8 192-root sample those rounds benched (a subset of the resident
    #     roots: bench_roots takes a prefix of one seeded permutation), so that the numbers of all rounds stay comparable
    cont = None
    if args.full and 0 < args.continuity_roots < R and world == 1:
        sub = workloads.bench_roots(rowptr, args.continuity_roots, rank, world, args.seed)
        slot_of = {int(r): i for i, r in enumerate(roots)}
        sub_slots = np.array([slot_of[int(r)] for r in sub], dtype=np.int32)

        def sub_step(i):
            rows = eng.prepare_d(sub_slots, args.seed, 2 * i, fetch=False)
            if not args.no_g_head_start:
                eng.prepare_g_begin(sub_slots, args.n_sample_gen, args.seed, 2 * i + 1)
            eng.d_pass(np.zeros(1, np.int64), max(int(rows), 1))
            pairs = eng.prepare_g(sub_slots, args.n_sample_gen, args.seed, 2 * i + 1, fetch=False)
            eng.g_pass(np.zeros(1, np.int64), max(int(pairs), 1))
        for i in range(nxt, nxt + 3):
            sub_step(i)
        barrier()
        cc0 = eng.counters()
        tc = time.perf_counter()
        for i in range(nxt + 3, nxt + 3 + args.steps):
            sub_step(i)
        barrier()
        dtc = time.perf_counter() - tc
        cc = delta(eng.counters(), cc0)
        cont = {"roots_per_step": int(len(sub)), "value": cc["hops"] / dtc, "unit": "edges/s", "ms_per_step": 1e3 * dtc / args.steps,
                "rows_scored_per_step": cc["rows_scored"] / args.steps,
                "what": "the same step over the %d-root sample rounds 1-2 benched (a subset of the resident roots)" % len(sub)}
        nxt += 3 + args.steps
    # (1) the same kernel events with the profiled side-stream launches ISOLATED (they first wait for the main stream): the
    #     kernel alone on the chip.  Not part of the timed region: isolating a launch serialises that step.
    co = None
    if args.full:
        eng.set_profiling_solo(True)
        eng.set_profiling(args.profile_every)
        c2 = eng.counters()
        for i in range(nxt, nxt + args.overlap_steps):
            step(i, head_start=False)  # (a head start would put the walks beside the D pass again: the launch has nothing to wait for yet)
        barrier()
        co = delta(eng.counters(), c2)
        eng.set_profiling_solo(False)
        nxt += args.overlap_steps
    # (2) end to end for roots whose trees are NOT resident: build the BFS trees of a fresh batch of R roots on the GPU,
    #     then one step on them (an epoch over all N roots is a sequence of exactly this)
    e2e = None
    if args.full and args.fresh_batches > 0 and not args.host_bfs:
        c3 = eng.counters()
        barrier()
        t3 = time.perf_counter()
        for k in range(args.fresh_batches):
            fresh = workloads.bench_roots(rowptr, args.roots, rank, world, args.seed + 101 + k)
            eng.build_trees(fresh, device=True)
            step(nxt + k)
        barrier()
        dt3 = time.perf_counter() - t3
        c4 = delta(eng.counters(), c3)
        e2e_whole = (c4["hops"], dt3, c4["bfs_kernel_ms"], c4["bfs_trees"])
        # ... and the same with LAZY trees (round 6; what gg_epoch_add builds by default on a graph of this size): exact through
        # the last level that fits a node limit, deeper children lists resolved by the walks that stand on them -- same walks, bit
        # for bit (tests/test_gpu_lazy.py, tools/lazy_time.py).  One untimed batch first: the lazy arrays are allocated there.
        eng.set_tree_mode(1)
        eng.build_trees(workloads.bench_roots(rowptr, args.roots, rank, world, args.seed + 201), device=True)
        step(nxt + args.fresh_batches)
        c3 = eng.counters()
        barrier()
        t3 = time.perf_counter()
        lz = []
        for k in range(args.fresh_batches):
            fresh = workloads.bench_roots(rowptr, args.roots, rank, world, args.seed + 301 + k)
            eng.build_trees(fresh, device=True)
            step(nxt + args.fresh_batches + 1 + k)
            lz.append(eng.lazy_stats())
        barrier()
        dt3 = time.perf_counter() - t3
        c4 = delta(eng.counters(), c3)
        e2e = (c4["hops"], dt3, c4["bfs_kernel_ms"], c4["bfs_trees"], lz)
        eng.set_tree_mode(-1)

    hops, reads, rows_scored = c["hops"], c["nbr_reads"], c["rows_scored"]
    walk_ms, launches = c["walk_kernel_ms"], c["walk_launches"]  # HIP events of the profiled walk launches and how many that was
    calls = 2 * args.steps
    sums = ctl.sum([hops, c["d_pairs"], c["g_pairs"], e2e[0] if e2e else 0.0, e2e_whole[0] if e2e else 0.0])
    tot = np.array([sums[0], sums[1], sums[2], ctl.max(dt)])
    e2e_dt = ctl.max(e2e[1]) if e2e else 0.0
    e2e_whole_dt = ctl.max(e2e_whole[1]) if e2e else 0.0
    if rank != 0:
        eng.close()
        return

    d = eng.n_emb

    def gbs(nbytes, ms):
        return nbytes / (ms * 1e-3) / 1e9 if ms > 0 else None

    def frac(x):
        return x / HBM_PEAK_GBS if x else None

    # K1, dominant kernel level_score_kernel.  Algorithmic bytes as SURVEY.md section 8d defines them: per candidate row
    # scored 4(d+2) (id + embedding row + bias), per evaluated (root, node) distribution 4d+12 (ONE current row, tree
    # pointers, output id); rows / distributions / milliseconds / launches are counted over the same profiled launches.
    # (The kernel re-reads the current row once per 16-candidate work item and writes scores: that is traffic, not algorithm.)
    def k1(cc):
        b = 4.0 * (d + 2) * cc["score_rows"] + (4.0 * d + 12.0) * cc["score_dists"]
        return b, gbs(b, cc["score_kernel_ms"])

    sc_bytes, achieved = k1(c)
    _, achieved_ovl = k1(co) if co else (None, None)
    sc_launches = c["score_launches"]
    # The reference evaluates every hop's distribution from scratch (4k(d+2) + 4d + 12 per hop);
    # the engine evaluates each distinct (root, node) distribution of a launch once.
    ref_bytes = 4.0 * (d + 2) * reads + (4.0 * d + 12.0) * hops
    big_default = args.workload == "powerlaw" and args.nodes == 1_000_000 and args.emb == 128 and args.roots == 16384  # what the committed PMC passes ran
    traffic, traffic_src = pmc_traffic("level_score_kernel") if big_default else (None, None)
    # K2 pair_reward: 8d + 16 per pair.  K3 / K4 (fast mode, lazy Adam) per section 8d: gradient kernel 16d + 20 per pair
    # (two rows read, two rows of gradient added), whole step 48d + 36 per pair; K5 optimizer kernel per touched row:
    # E, m, v read + written, gradient read + cleared = 32d, plus 32 for the bias and its slots.
    row_b = 32.0 * d + 32.0 if args.optimizer != "sgd" else 16.0 * d + 16.0
    k2_pair_model = gbs((8.0 * d + 16.0) * c["reward_pairs_timed"], c["reward_kernel_ms"])
    # path_reward_kernel reads every path node's row once per walk (row + id + bias) and writes one reward per pair
    k2 = gbs((4.0 * d + 8.0) * c["g_walk_nodes_timed"] + 4.0 * c["reward_pairs_timed"], c["reward_kernel_ms"])

    def by_traffic(kernel, ms, launches):
        t, src = pmc_traffic(kernel) if big_default else (None, None)
        if not t or not launches or ms <= 0:
            return {"traffic": None}
        v = gbs(t * launches, ms)
        return {"traffic": t, "traffic_source": src, "traffic_GBs": v, "traffic_frac": frac(v)}
    kd_g = gbs((16.0 * d + 20.0) * c["d_pairs_timed"], c["d_grad_ms"])
    kg_g = gbs((16.0 * d + 20.0) * c["g_pairs_timed"], c["g_grad_ms"])
    # G pass, staged gradient (single replica): the gradient kernel reads every path node's row once and stores one staged
    # row per node (8d + 16 per node); the reducing optimizer reads the staged rows (4d + 4 each) and reads + writes E, m, v
    # of every touched row (24d + 24; no accumulator round trip)
    nodes_per_pair = c["g_walk_nodes_timed"] / c["reward_pairs_timed"] if c["reward_pairs_timed"] else 0.0
    g_nodes = nodes_per_pair * c["g_pairs_timed"]
    staged = world == 1 and args.optimizer != "adam_dense" and not os.environ.get("GG_NO_STAGED_GRAD") and os.environ.get("GG_STAGE_T") != "0"
    kg_nodes = gbs((8.0 * d + 16.0) * g_nodes, c["g_grad_ms"])
    row_st = 24.0 * d + 24.0 if args.optimizer != "sgd" else 8.0 * d + 8.0
    if staged:
        kg_o = gbs(row_st * c["g_rows_timed"] + (4.0 * d + 4.0) * g_nodes, c["g_opt_ms"])
        # D pass: one staged row per pair (v side) + one per run of equal centres inside 16 pairs (u side)
        kd_o = gbs(row_st * c["d_rows_timed"] + (4.0 * d + 4.0) * c["d_pairs_timed"] * (1.0 + 1.0 / 16.0), c["d_opt_ms"])
    else:
        kg_o = gbs(row_b * c["g_rows_timed"], c["g_opt_ms"])
        kd_o = gbs(row_b * c["d_rows_timed"], c["d_opt_ms"])
    kd_s = gbs((48.0 * d + 36.0) * c["d_pairs_timed"], c["d_grad_ms"] + c["d_opt_ms"])
    # the same pass in the old call order (steps behind the timed region): the G-mode walks start later, the kernel runs (almost) alone
    kd_g_solo = gbs((16.0 * d + 20.0) * co["d_pairs_timed"], co["d_grad_ms"]) if co and co.get("d_passes_timed") else None
    kg_s = gbs((48.0 * d + 36.0) * c["g_pairs_timed"], c["g_grad_ms"] + c["g_opt_ms"])
    out = {
        "metric": "sampled_edges_per_sec",
        "value": tot[0] / tot[3],
        "unit": "edges/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1e3 * tot[3] / args.steps,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": wl_name, "roots_per_gpu_per_step": int(R), "n_sample_gen": args.n_sample_gen,
                   "optimizer": args.optimizer, "step": "prepare_d + d_pass + prepare_g + g_pass (graph_gan.py:144-176, one inner pass each)" + ("" if args.no_g_head_start else "; the walks of prepare_g are enqueued before d_pass (gg_prepare_g_begin)"),
                   "parallelism": ("roots sharded x%d, replicated tables, RCCL gradient exchange per pass: %s" % (world, exchange_label(comm))) if world > 1 else "single GPU"},
        # pairs through the update kernels / HIP-event time of those kernels (gradient + optimizer) on the profiled passes
        "d_step_pairs_per_sec": c["d_pairs_timed"] / ((c["d_grad_ms"] + c["d_opt_ms"]) * 1e-3) if c["d_grad_ms"] > 0 else None,
        "g_step_pairs_per_sec": c["g_pairs_timed"] / ((c["g_grad_ms"] + c["g_opt_ms"]) * 1e-3) if c["g_grad_ms"] > 0 else None,
        "d_pairs_per_step_all_ranks": tot[1] / args.steps,
        "g_pairs_per_step_all_ranks": tot[2] / args.steps,
        "walk_kernel_edges_per_sec": (hops / calls) / (walk_ms / launches * 1e-3) if walk_ms > 0 and launches else None,
        "hops_per_step_rank0": hops / args.steps,
        "mean_k": reads / max(hops, 1),
        "rows_scored_per_step_rank0": rows_scored / args.steps,
        "walk_reruns_in_timed_region": c["walk_reruns"],  # sync-free launches repeated in sized mode (0 in steady state)
        "edge_score_cache": {"distributions_gathered_per_step": c["es_gathers"] / args.steps, "nodes_scored_whole_per_step": c["es_nodes"] / args.steps,
                             "what": "s(u, v) of a graph edge does not depend on the root: a node's adjacency is scored once per generator state "
                                     "and shared by the (root, node) distributions of all roots, levels and both walk launches of a step"},
        "nbr_reads_per_step_rank0": reads / args.steps,
        "setup_s": setup_s,
        "tree_build": {"where": "host threads" if args.host_bfs else "gpu bfs (one workgroup per root, visited bitmap in LDS)", "trees": int(R), "call_s": trees_s,
                       "kernel_ms": c_trees["bfs_kernel_ms"], "us_per_tree": 1e3 * c_trees["bfs_kernel_ms"] / max(c_trees["bfs_trees"], 1) if c_trees["bfs_trees"] else None,
                       "resident_bytes_per_tree": 12.0 * n},
        "roofline": {"kernel": "level_score_kernel", "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": frac(achieved), "traffic": traffic, "traffic_source": traffic_src,
                     "traffic_same_run": (dict(pmc_same_run(), traffic=traffic, traffic_over_algorithmic=traffic / pmc_same_run()["algorithmic_bytes_per_launch"])
                                          if big_default and traffic and pmc_same_run() else None),
                     "algorithmic_bytes_per_launch": sc_bytes / max(sc_launches, 1), "avg_launch_ms": c["score_kernel_ms"] / max(sc_launches, 1),
                     "launches": int(sc_launches), "rows_per_launch": c["score_rows"] / max(sc_launches, 1),
                     "distributions_per_launch": c["score_dists"] / max(sc_launches, 1),
                     "bytes_model": "SURVEY 8d: 4(d+2) per candidate row scored + (4d+12) per scoring task that reads a current row (a private (root, node) "
                                    "distribution, or a node whose whole adjacency is scored once into the edge-score cache for every root)",
                     "timed": "HIP events on the engine's stream around every level_score_kernel launch of every %s walk call of the timed region, "
                              "as it runs in production: the G-mode launches share the chip with the discriminator update on the other stream" % (
                                  "" if args.profile_every == 1 else "%d-th" % args.profile_every),
                     "solo": ({"achieved": achieved_ovl, "frac": frac(achieved_ovl), "launches": int(co["score_launches"]),
                               "what": "%d further steps whose profiled side-stream launches first wait for the main stream (the kernel alone on the chip)" % args.overlap_steps}
                              if co else None),
                     # the sampler as a WHOLE: the same algorithmic bytes over the whole walk launches (score + weights + advance +
                     # the small kernels around them), HIP events around the profiled launches -- the level glue is latency bound and
                     # moves few algorithmic bytes, so this fraction is about half the score kernel's
                     "whole_sampler": ({"achieved": sc_bytes / (walk_ms * 1e-3) / 1e9, "frac": frac(sc_bytes / (walk_ms * 1e-3) / 1e9), "ms_per_walk_call": walk_ms / launches,
                                        "what": "SURVEY 8d bytes of the profiled walk launches / their whole event time (every kernel of gg_walk_sample's launch)"}
                                       if walk_ms > 0 and launches and c["score_launches"] else None),
                     "microbenchmarks": "profiles/r1_gather_bw2.txt, profiles/r1_gather_bw3.txt (tools/gather_bw*.hip on the same chip)"},
        "roofline_k2": {"kernel": "path_reward_kernel", "bound": "hbm", "achieved": k2, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": frac(k2),
                        "bytes_model": "(4d + 8) per path node + 4 per pair: the whole-walk kernel reads every row once per walk",
                        "per_pair_model": {"bytes_model": "SURVEY 8d: 8d + 16 per pair", "achieved": k2_pair_model,
                                           "note": "above the HBM peak by construction: the 2-8 uses of a row by the window pairs of its walk come from registers"},
                        "pairs": int(c["reward_pairs_timed"]), "path_nodes": int(c["g_walk_nodes_timed"]), "ms": c["reward_kernel_ms"]},
        "roofline_k34": {"bound": "hbm (fp32 atomics in L2)", "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "bytes_model": "gradient kernel 16d + 20 per pair; whole step (gradient + optimizer) 48d + 36 per pair (SURVEY 8d, lazy Adam); "
                                        "traffic_* = HBM bytes of the PMC passes / the same event time: what the atomics really move",
                         "d": dict({"kernel": "pair_grad16_kernel (+ count / segment / slot kernels when staged)", "staged": bool(staged), "achieved": kd_g, "frac": frac(kd_g), "step_achieved": kd_s, "step_frac": frac(kd_s),
                                    "pairs": int(c["d_pairs_timed"]), "grad_ms": c["d_grad_ms"], "passes": int(c["d_passes_timed"]),
                                    "timed": "as it runs in production: beside the G-mode walks" + ("" if args.no_g_head_start else ", which gg_prepare_g_begin starts before the pass"),
                                    "without_head_start": ({"achieved": kd_g_solo, "frac": frac(kd_g_solo), "passes": int(co.get("d_passes_timed", 0)),
                                                            "what": "the %d steps behind the timed region, which run in the old call order: the G-mode walks start once the host has enqueued the pass, "
                                                                    "so the gradient kernel has the chip (almost) to itself" % args.overlap_steps}
                                                           if co else None)},
                                   **by_traffic("pair_grad16_kernel", c["d_grad_ms"], c["d_passes_timed"])),
                         "g": dict({"kernel": "path_grad_kernel (+ count / segment / slot kernels when staged): reads every path node once and emits one gradient row per node",
                                    "bytes_model": "8d + 16 per path node (row read + gradient row written)", "path_nodes": int(g_nodes),
                                    "achieved": kg_nodes, "frac": frac(kg_nodes), "pairs": int(c["g_pairs_timed"]),
                                    "grad_ms": c["g_grad_ms"], "passes": int(c["g_passes_timed"]), "staged": bool(staged),
                                    "per_pair_model": {"bytes_model": "SURVEY 8d: 16d + 20 per pair, whole step 48d + 36", "achieved": kg_g, "step_achieved": kg_s,
                                                       "note": "above the HBM peak by construction: a row serves the 2-8 window pairs of its walk from registers"}},
                                   **by_traffic("path_grad_kernel", c["g_grad_ms"], c["g_passes_timed"]))},
        "roofline_opt": {"kernel": "sparse_opt_kernel (+ flag scan / compaction%s)" % (", replica exchange" if world > 1 else ""), "bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "bytes_model": "%s per touched row" % ("32d + 32 (E, m, v read + written, gradient read + cleared)" if args.optimizer != "sgd" else "16d + 16"),
                         "d": {"achieved": kd_o, "frac": frac(kd_o), "rows": int(c["d_rows_timed"]), "ms": c["d_opt_ms"],
                               "bytes_model": ("staged_opt_kernel: 24d + 24 per touched row + 4d + 4 per staged gradient row (pairs x 17/16)" if staged else "32d + 32 per touched row")},
                         "g": {"achieved": kg_o, "frac": frac(kg_o), "rows": int(c["g_rows_timed"]), "ms": c["g_opt_ms"],
                               "bytes_model": ("staged_opt_kernel: 24d + 24 per touched row (E, m, v read + written) + 4d + 4 per staged gradient row" if staged else "as d")}},
        "walk_phase": {"ms_per_walk_sample_call": walk_ms / max(launches, 1), "calls": calls, "calls_timed": int(launches),
                       "reference_equivalent_bytes_per_call": ref_bytes / calls,
                       "reference_equivalent_GBs": (ref_bytes / calls) / (walk_ms / launches * 1e-3) / 1e9 if walk_ms > 0 and launches else None,
                       "distributions_shared": reads / max(rows_scored, 1)},
    }
    # ---- the tree build.  NOT priced against the HBM peak any more (round-4 verdict): one workgroup builds one tree with its visited
    # bitmap in LDS (122 KB at 10^6 nodes: one workgroup per compute unit, 4 wavefronts per SIMD), 256 trees at a time share the
    # adjacency (48 MB: it lives in the 256 MB Infinity Cache, FETCH_SIZE is ~78 MB per tree against 108 MB "algorithmic"), and what a
    # tree costs is its compute unit's time: dependent LDS operations per adjacency entry (bit test, atomic-or claim, duplicate
    # hash, popcount prefix) at a third of the issue slots.  Quoted as microseconds per tree and compute-unit cycles per entry.
    nnz = int(rowptr[-1])
    bfs_us = out["tree_build"]["us_per_tree"]
    cu_cycles = bfs_us * 1e-6 * N_CU * ENGINE_CLOCK_HZ if bfs_us else None  # one CU is busy N_CU x (time per tree) per tree
    out["tree_build"].update({"cu_cycles_per_tree": cu_cycles,
                              "cu_cycles_per_adjacency_entry": cu_cycles / nnz if cu_cycles else None,
                              "cu_cycles_per_node": cu_cycles / n if cu_cycles else None,
                              "bound": "one workgroup per CU beside a %d KB LDS bitmap: latency of dependent LDS operations, not HBM (adjacency %.0f MB, resident in the Infinity Cache across the %d concurrent roots)"
                                       % ((n + 7) // 8 // 1024, 4.0 * nnz / 1e6, N_CU),
                              "assumed": {"compute_units": N_CU, "engine_clock_hz": ENGINE_CLOCK_HZ}})
    # (scalars: the driver's record keeps the scalar members of `roofline` and `config`)
    out["roofline"]["bfs_us_per_tree"] = bfs_us
    out["roofline"]["bfs_cu_cycles_per_adjacency_entry"] = out["tree_build"]["cu_cycles_per_adjacency_entry"]
    if cont:
        out["batch_of_rounds_1_2"] = cont
    if c["d_passes_timed"] and c["g_passes_timed"]:
        d_pass_ms = (c["d_grad_ms"] + c["d_opt_ms"]) / c["d_passes_timed"]
        g_pass_ms = (c["g_grad_ms"] + c["g_opt_ms"]) / c["g_passes_timed"] if c["g_passes_timed"] else None
        out["comm_model"] = dict(comm_model(n, eng.n_emb + (-eng.n_emb) % 4, c["d_rows_timed"] / c["d_passes_timed"], c["g_rows_timed"] / c["g_passes_timed"],
                                            c["d_pairs"] / args.steps, c["g_pairs"] / args.steps, step_ms=1e3 * dt / args.steps, d_pass_ms=d_pass_ms,
                                            g_walk_ms=walk_ms / launches if launches else None,
                                            epoch=(dict(n_roots=n, n_batches=n / float(R), pass_s_per_batch=1e-3 * (d_pass_ms + g_pass_ms),
                                                        prepare_s_per_batch=max(e2e_dt / args.fresh_batches - 1e-3 * (d_pass_ms + g_pass_ms), 0.0))
                                                   if e2e and d_pass_ms is not None and g_pass_ms is not None else None)),
                                 what="bytes one rank would send per step for its two gradient exchanges, from this run's per-rank touched rows / pairs "
                                      "(unit B), the time they would take on xGMI and the weak-scaling efficiency that follows; a MODEL, NOT measured "
                                      "(no multi-GPU box has run this code)")
    if comm:
        out["comm"] = dict(comm, what="rank 0's gradient exchanges up to the end of the timed region (RCCL over xGMI): optimizer steps that exchanged "
                                      "fixed-capacity row packs (sparse) / reduce-scatter + all-gather of the accumulators (dense), bytes sent")
    if e2e:
        lzs = e2e[4]
        out["end_to_end_with_tree_build"] = {
            "value": sums[3] / e2e_dt, "unit": "edges/s",
            "what": "%d fresh batches of %d roots per GPU: gg_build_trees_device (LAZY trees: exact through the last level that fits the node "
                    "limit, deeper children lists resolved by the walks) + one step each (trees not resident)" % (args.fresh_batches, R),
            "s_per_batch": e2e_dt / args.fresh_batches, "bfs_kernel_ms_per_batch": e2e[2] / args.fresh_batches,
            "bfs_us_per_tree": 1e3 * e2e[2] / max(e2e[3], 1),
            "slots_rebuilt_whole_per_batch": (lzs[-1]["fallback_roots"] - 0) / (args.fresh_batches + 1.0),
            "exact_nodes_per_root": float(np.mean([z["exact_nodes"] for z in lzs])) / R, "pool_entries_per_root": float(np.mean([z["pool_entries"] for z in lzs])) / R,
            "lazy_slots_by_exact_level": lzs[-1]["slots_by_level"]}
        out["end_to_end_with_tree_build_whole_trees"] = {
            "value": sums[4] / e2e_whole_dt, "unit": "edges/s",
            "what": "the same with whole trees (rounds 2-5: every root's BFS to its last node)",
            "s_per_batch": e2e_whole_dt / args.fresh_batches, "bfs_kernel_ms_per_batch": e2e_whole[2] / args.fresh_batches,
            "bfs_us_per_tree": 1e3 * e2e_whole[2] / max(e2e_whole[3], 1)}
        # the number a user of this configuration sees when the trees are NOT resident (an epoch over all N roots is a
        # sequence of exactly these batches): beside the resident-trees headline, where the driver's record keeps it
        out["roofline"]["with_tree_build_edges_per_sec"] = sums[3] / e2e_dt
        out["config"]["with_tree_build_edges_per_sec"] = sums[3] / e2e_dt
        out["config"]["with_tree_build_s_per_batch"] = e2e_dt / args.fresh_batches
    if args.full and world == 1 and not args.no_strict:
        out["strict_mode"] = strict_mode_line(ga, _lib)
        out["strict_mode_1m"] = strict_mode_at_scale(ga, _lib, n, rowptr, col, emb, roots[:2048], args.n_sample_gen, args.seed)
        out["config"]["pairs_per_sec_batching"] = ("d_step_pairs_per_sec / g_step_pairs_per_sec: one fused batch per pass (fast mode, SURVEY 8d 2(ii)); "
                                                   "the reference's batch-64 schedule on this graph: strict_mode_1m")
    if args.full and world == 1 and not args.no_cpu_baseline:
        bias = eng.get_bias(0)
        embg = eng.get_embeddings(0)
        v, sample = cpu_baseline(args, n, rowptr, col, embg, bias, roots, args.cpu_baseline_seconds)
        one_core = {"value": v, "unit": "edges/s", "cores": 1, "host_cores_on_box": os.cpu_count(), "kind": "port", "sample": sample}
        out["walk_kernel_vs_cpu"] = out["walk_kernel_edges_per_sec"] / v if v > 0 and out["walk_kernel_edges_per_sec"] else None
        # `cpu_baseline` = the same port on MANY host cores (the north star's "timed on the same box's host cores, core count stated");
        # the one-core figure stays beside it.  A failure of the threaded leg never costs the bench line: the one-core figure stands in.
        try:
            many = cpu_baseline_threads(args, n, rowptr, col, embg, bias, roots, 8.0, min(64, max(1, (os.cpu_count() or 2) // 2)))
        except Exception as e:  # noqa: BLE001
            many = {"error": repr(e)}
        out["cpu_baseline"] = many if "value" in many else one_core
        out["cpu_baseline_one_core"] = one_core
        out["cpu_baseline_all_cores"] = many  # (the key of round 5's records)
        out["cpu_baseline_faithful"] = cpu_baseline_faithful()
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
