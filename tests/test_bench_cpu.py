"""CPU-side pieces of bench.py (no GPU): the faithful CPU baseline leg, the PMC-summary lookup, the defaults the driver
relies on (`python bench.py` with no flags = 1 GPU, a few timed steps)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_defaults_and_faithful_baseline(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse()
    from graphgan_amd import workloads
    assert a.roots == workloads.BENCH_ROOTS and a.continuity_roots == workloads.BENCH_ROOTS_ROUND2
    assert a.gpus == 1 and 1 <= a.steps <= 50 and a.warmup >= 1 and a.nodes == 1_000_000 and a.emb == 128
    r = bench.cpu_baseline_faithful(2)  # two all_score recomputations on CA-GrQc + the C oracle's walks
    assert r["value"] > 0 and r["unit"] == "edges/s" and r["kind"] == "port" and "faithful" in r["flavour"]


def test_pmc_summary_lookup_takes_the_latest_round():
    import bench
    traffic, src = bench.pmc_traffic("level_score_kernel")
    files = sorted(f for f in os.listdir(os.path.join(ROOT, "profiles")) if f.endswith("_pmc_hbm_traffic.json"))
    assert src == os.path.join("profiles", files[-1]) and traffic > 1e8
    data = json.load(open(os.path.join(ROOT, src)))
    assert any("level_score_kernel" in k for k in data)
    assert bench.pmc_traffic("no_such_kernel") == (None, None)


def test_gpus_n_launches_its_own_ranks(tmp_path, monkeypatch):
    """`python bench.py --gpus N` with no launcher around it starts N ranks itself (it used to exit): every rank
    gets the environment torch.distributed.run would export, rank 0's stdout is the bench's stdout, a failing rank fails
    the whole run.  The ranks here are a stand-in script (no GPU in this container)."""
    import subprocess
    import bench
    child = tmp_path / "child.py"
    child.write_text(
        "import json, os, sys\n"
        "r = int(os.environ['RANK'])\n"
        "open(os.path.join(os.path.dirname(__file__), 'rank%d' % r), 'w').write(' '.join(sys.argv[1:]))\n"
        "print(json.dumps({k: os.environ[k] for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}))\n"
        "sys.exit(int(os.environ.get('CHILD_FAIL_RANK', '-1')) == r)\n")
    driver = ("import sys; sys.argv = ['bench.py', '--gpus', '3', '--steps', '2']; sys.path.insert(0, %r); import bench; "
              "bench.self_launch(3, %r)" % (ROOT, str(child)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "-c", driver], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    line = json.loads(r.stdout)   # exactly one line: rank 0's
    assert line["RANK"] == "0" and line["WORLD_SIZE"] == "3" and line["MASTER_ADDR"] == "127.0.0.1" and int(line["MASTER_PORT"]) > 0
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("rank")) == ["rank0", "rank1", "rank2"]
    assert (tmp_path / "rank2").read_text() == "--gpus 3 --steps 2"
    r = subprocess.run([sys.executable, "-c", driver], capture_output=True, text=True, env=dict(env, CHILD_FAIL_RANK="1"), timeout=120)
    assert r.returncode != 0 and "rank exit codes [0, 1, 0]" in r.stderr
    # main() takes that path exactly when no launcher exported WORLD_SIZE
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert 'if "WORLD_SIZE" not in os.environ and args.gpus > 1:' in src and "must be launched with" not in src


def test_comm_model_prices_the_exchange_on_xgmi():
    """bench.comm_model: bytes per strategy, the time they take over P - 1 point-to-point links, what stays exposed and the
    weak-scaling efficiency that follows (a MODEL: no multi-GPU run exists).  Sanity of its arithmetic on the bench's counts."""
    import bench
    m = bench.comm_model(1_000_000, 128, 445_000, 488_000, 646_000, 3_630_000, step_ms=4.05, d_pass_ms=1.1, g_walk_ms=1.34)
    row = 4.0 * 130
    for P in (2, 4, 8):
        e = m["P=%d" % P]
        f = (P - 1.0) / P
        want = sum(f * t * row + f * min(1_000_000, P * t) * row for t in (445_000, 488_000))
        assert abs(e["owner_partitioned_sparse"] - want) < 1.0
        assert e["owner_partitioned_sparse_bf16"] < 0.52 * e["owner_partitioned_sparse"]           # half the row bytes (+ the ids)
        t32, t16 = e["modelled_time_owner_fp32"], e["modelled_time_owner_bf16"]
        rate = (P - 1) * bench.XGMI_LINK_GBS * 1e9 * bench.XGMI_EFFICIENCY
        assert abs(t32["d_exchange_ms"] + t32["g_exchange_ms"] - (1e3 * want / rate + 4 * bench.HOST_ROUND_TRIP_MS)) < 1e-9
        # the D exchange hides behind the G-mode walks as far as they reach; the G exchange is exposed in full
        assert abs(t32["exposed_ms_per_step"] - (max(0.0, 1.1 + t32["d_exchange_ms"] - 1.34) + t32["g_exchange_ms"])) < 1e-12
        assert 0.0 < t32["weak_scaling_efficiency_estimate"] < t16["weak_scaling_efficiency_estimate"] < 1.0
    assert m["P=8"]["modelled_time_owner_fp32"]["weak_scaling_efficiency_estimate"] < 0.8     # not near-linear at this batch: said so in DESIGN section 7
    assert m["assumptions"]["xgmi_link_GBs"] == 153.0


def test_dump_outputs_writes_fixed_samples_of_the_last_step(tmp_path, monkeypatch):
    """`--dump-outputs DIR` (off by default, like `--full`): both models' table rows and biases, the D rows and the G pairs
    of the last step as float32 / float64 .npy files -- the same seeded sample on every run, under 64 MB in all.  The
    engine is a stand-in with the Engine's getters (no GPU in this container)."""
    import numpy as np
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None

    n, d = 50_000, 128
    rs = np.random.RandomState(3)

    class Eng:
        n_node, n_emb = n, d
        emb = [rs.rand(n, d).astype(np.float32) for _ in range(2)]
        d_data = (rs.randint(0, n, 300_000).astype(np.int32), rs.randint(0, n, 300_000).astype(np.int32), (rs.rand(300_000) < 0.5).astype(np.float32))
        g_data = (rs.randint(0, n, 1000).astype(np.int32), rs.randint(0, n, 1000).astype(np.int32), rs.rand(1000).astype(np.float32))

        def get_embeddings(self, which):
            return self.emb[which].copy()

        def get_bias(self, which):
            return np.arange(self.n_node, dtype=np.float32) + 0.5 * which

        def get_d_data(self):
            return self.d_data

        def get_g_data(self):
            return self.g_data

    eng = Eng()
    bench.dump_outputs(eng, str(tmp_path / "a"))
    bench.dump_outputs(eng, str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(k + ".npy" for k in ("gen_emb_rows", "gen_bias_rows", "dis_emb_rows", "dis_bias_rows", "d_center", "d_neighbor",
                                                "d_label", "g_node_1", "g_node_2", "g_reward"))
    out = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n, v in out.items():
        assert v.dtype in (np.float32, np.float64), n
        assert np.array_equal(v, np.load(tmp_path / "b" / (n + ".npy"))), n   # the same sample on every run
    assert sum(v.nbytes for v in out.values()) <= 64 << 20
    rows = out["gen_bias_rows"].astype(np.int64)   # the bias of node i is i here: the sampled node ids
    assert len(rows) == bench.DUMP_TABLE_BYTES // (4 * Eng.n_emb) and np.all(np.diff(rows) > 0)
    assert np.array_equal(out["gen_emb_rows"], Eng.emb[0][rows]) and np.array_equal(out["dis_emb_rows"], Eng.emb[1][rows])
    assert np.array_equal(out["dis_bias_rows"], rows + 0.5)
    assert len(out["d_center"]) == bench.DUMP_PAIRS and set(out["d_label"]) <= {0.0, 1.0}
    assert np.array_equal(out["g_node_1"], Eng.g_data[0]) and np.array_equal(out["g_reward"], Eng.g_data[2])   # below the cap: all pairs


def test_full_and_dump_outputs_combine_with_the_legs_flags(tmp_path, monkeypatch):
    """--full / --dump-outputs parse together with the flags of the legs they gate; a narrow table keeps the dump small."""
    import numpy as np
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out", "--no-cpu-baseline", "--no-strict", "--fresh-batches", "1",
                                      "--overlap-steps", "2", "--continuity-roots", "512", "--steps", "7"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out" and a.no_cpu_baseline and a.no_strict and a.fresh_batches == 1 and a.overlap_steps == 2
    assert a.continuity_roots == 512 and a.steps == 7

    class Narrow:  # d = 1 and many nodes: the row sample is capped, not only by bytes per table
        n_node, n_emb = 5_000_000, 1

        def get_embeddings(self, which):
            return np.zeros((self.n_node, 1), np.float32)

        def get_bias(self, which):
            return np.zeros(self.n_node, np.float32)

        def get_d_data(self):
            return np.zeros(10, np.int32), np.zeros(10, np.int32), np.zeros(10, np.float32)

        def get_g_data(self):
            return np.zeros(10, np.int32), np.zeros(10, np.int32), np.zeros(10, np.float32)
    bench.dump_outputs(Narrow(), str(tmp_path))
    sizes = {n: os.path.getsize(tmp_path / n) for n in os.listdir(tmp_path)}
    assert sum(sizes.values()) < 64 << 20 and np.load(tmp_path / "gen_bias_rows.npy").shape == (bench.DUMP_TABLE_ROWS,)
