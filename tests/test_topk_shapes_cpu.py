"""The premises of tests/test_gpu_topk_lists.py and tests/test_gpu_rank_lists.py, checked without a GPU: the restated plans of
the top-K and the rank consumer (tests/support/topk_shapes.py) give the long column splits the cases are named for, the
programmed tables are exact in fp32 and in bf16 and their query rows ARE the programs, the model of the per-wavefront lists
agrees with the lexsort reference, and -- in the model -- every row program drives the path of wave_insert it is named for and
the k best columns of a homed program all come out of one wavefront's list.  The last are conditions on the inputs, not
measurements of the device."""
import os

import numpy as np
import pytest

from tests.support import topk_shapes as ts

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graphgan_amd", "csrc")


def test_plan_restatement_still_stands_in_the_source():
    # drift guard: tests/support/topk_shapes.py restates these lines.  If this fails after an edit of the kernels' files the
    # plan, the work split or the list layout may have changed: update the restatement (or, after a mere reformat, these texts)
    topk = open(os.path.join(CSRC, "topk_score.hip")).read()
    for text in ("constexpr int TK_CHUNK = 4096;",
                 "constexpr int TK_MAX_K = 256;",
                 "constexpr size_t TK_PART_CAP = size_t(256) << 20;",
                 "const int chunk = std::min(n_rows, TK_CHUNK);",
                 "const ColumnSplit cs = column_split(n, cdiv(chunk, 32), 2048, (int)(TK_PART_CAP / ((size_t)chunk * 4 * k * sizeof(u64))));",
                 "const int split = blockIdx.x, r0 = blockIdx.y * 32, sub = 4 * split + (threadIdx.x >> 6);",
                 "const int cbeg = split * cols_per_split, cend = min(n_node, cbeg + cols_per_split);",
                 "const bool p = ok && x >= t;",
                 "if (heads[j] <= cur[k - 1]) continue;",
                 "const size_t dyn = sizeof(float) * 32 * (size_t)(ld + 1);",
                 "if (precision == 0 && dyn > 48 * 1024) (void)hipFuncSetAttribute((const void *)topk_f32_kernel"):
        assert text in topk, "topk_score.hip no longer contains %r: restate it in tests/support/topk_shapes.py" % text
    rank = open(os.path.join(CSRC, "rank_score.hip")).read()
    for text in ("constexpr int RK_CHUNK = 4096;",
                 "const int chunk = (int)std::min<int64_t>(m, RK_CHUNK);",
                 "const ColumnSplit cs = column_split(n, cdiv(chunk, 32), 2048);",
                 "return x > t || (x == t && c < v);",
                 "if (precision == 0 && dyn > 48 * 1024) (void)hipFuncSetAttribute((const void *)rank_f32_kernel"):
        assert text in rank, "rank_score.hip no longer contains %r: restate it in tests/support/topk_shapes.py" % text
    tiles = open(os.path.join(CSRC, "score_tiles.h")).read()
    for text in ("for (int c0 = cbeg; c0 < cend; c0 += 128) {",
                 "const int col = c0 + wv * 32 + (lane & 31);",
                 "for (int c0 = cbeg + wv * 32; c0 < cend; c0 += 128) {",
                 "const int col = c0 + (lane & 31);"):
        assert text in tiles, "score_tiles.h no longer contains %r: restate it in tests/support/topk_shapes.py" % text
    assert "ctx->ld = (n_emb + 3) / 4 * 4;" in open(os.path.join(CSRC, "gg_api.hip")).read()


def test_restated_plans_give_the_long_splits():
    assert ts.topk_plan(ts.N_LONG, ts.N_ROWS, 256) == (8, 3072)
    assert ts.topk_plan(ts.N_INST, ts.N_ROWS, 255) == (8, 1152) and ts.N_INST % 1152 != 0   # a partial last split
    assert ts.topk_plan(ts.N_INST, ts.N_ROWS, 65) == (15, 640)
    assert ts.topk_plan(3000, 3000, 7) == (12, 256)
    assert ts.max_cols_per_wave(ts.N_LONG, 3072) == 768 and ts.max_cols_per_wave(ts.N_INST, 1152) == 288
    # the long case: a wavefront sees at least 3 k columns at every k, so every list fills and is inserted into afterwards
    for k in ts.KS_LONG:
        splits, cps = ts.topk_plan(ts.N_LONG, ts.N_ROWS, k)
        assert cps // 4 >= 3 * k and cps // 4 >= 384, (k, splits, cps)
    for n, d, k in ts.INSTANCE_CASES:
        splits, cps = ts.topk_plan(n, ts.N_ROWS, k)
        assert cps // 4 >= ts.k0_of(k) + 32, (n, k, cps)                                 # at least one tile behind the fill
    assert ts.rank_plan(ts.N_LONG, 4096) == (16, 1536) and ts.rank_plan(ts.N_LONG, 40) == (192, 128)
    assert ts.rank_plan(ts.N_INST, 4096) == (15, 640) and ts.rank_plan(ts.N_INST, 40) == (71, 128)
    # where(): the columns of a 128-column tile go to the 4 wavefronts 32 by 32, a wavefront's sequence grows with the column
    assert [ts.where(3072, c) for c in (0, 31, 32, 127, 128, 3071, 3072, 3072 + 128 * 5 + 70)] == \
        [(0, 0, 0), (0, 0, 31), (0, 1, 0), (0, 3, 31), (0, 0, 32), (0, 3, 767), (1, 0, 0), (1, 2, 166)]
    for (s, w), seq in ts.wave_columns(ts.N_INST, 1152).items():
        assert all(ts.where(1152, int(c)) == (s, w, i) for i, c in enumerate(seq))


def test_existing_tests_never_fill_a_long_list():
    """what the shapes of tests/test_gpu_topk.py and tests/test_gpu_rank.py reach (columns per wavefront = cols_per_split / 4)"""
    def cpw(n, rows, k):
        return ts.topk_plan(n, rows, k)[1] // 4
    for n in (700, 3000, 1029, 300, 600):                       # the fp32-exact and the bf16 test: 97 and 64 rows
        assert all(cpw(n, rows, k) == 32 for rows in (97, 64) for k in (1, 10, 100, 256))
    assert all(cpw(6000, 7, k) == 32 for k in (1, 7, 100, 256))  # ties
    assert cpw(34290, 7, 256) == 32 and cpw(34290, 1, 100) == 32  # the hub
    assert cpw(1000, 48, 256) == 32                              # test_rank_is_the_position_in_the_topk_list
    # the widest fast cases
    assert cpw(3000, 3000, 10) == 64 and cpw(3000, 3000, 256) == 96
    assert cpw(5000, 4500, 20) == 96 and cpw(5000, 5000, 5) == 96
    assert cpw(800, 40, 30) == 32 and cpw(300, 2, 10) == 32
    # a list with k >= 64 fills only at 10^6 (k = 100) and 10^7 nodes
    assert cpw(10 ** 6, 64, 100) == 256 and cpw(10 ** 7, 32, 100) > 256


CASES = ts.LONG_CASES + ts.INSTANCE_CASES


@pytest.mark.parametrize("n,d,k", CASES)
def test_tables_are_exact_and_their_query_rows_are_the_programs(n, d, k):
    c = ts.case(n, d, k)
    E, P = c["E"], c["P"]
    assert E.shape == (n, d) and P == (4 if d == 8 else 7) and c["names"] == ts.PROGRAMS[:P]
    assert np.array_equal(E, np.rint(E)) and np.abs(E).max() <= 256 and np.array_equal(ts.bf16_round(E), E)
    some = np.r_[c["qid"], np.random.RandomState(d).randint(0, n, 6)]
    G = ts.gram_rows(E, some)
    assert np.array_equal(G, E[some].astype(np.int64) @ E.astype(np.int64).T) and np.abs(G).max() < 2 ** 24
    # a bound for EVERY entry of E . E^T: the largest row norm squared
    assert (E.astype(np.int64) ** 2).sum(axis=1).max() < 2 ** 24
    for name, u in c["q"].items():
        s, j = c["S"][u], c["prog"][name]
        assert ts.where(c["cps"], u) == c["home"][j] + (0,) and not c["ordinary"][u]
        assert np.array_equal(s[c["ordinary"]], c["F"][j, c["ordinary"]]), name
        assert s[u] == ts.SELF and not s[np.setdiff1d(c["qid"], [u])].any()
    rows = c["rows"]
    assert len(rows) == ts.N_ROWS and set(rows.tolist()) == set(c["ids"].tolist()) and np.any(np.diff(rows) < 0)
    assert ts.bf16_shape(d) == {8: 4, 50: 4, 128: 8, 256: 16, 300: 32, 380: 32, 384: 32, 512: 32}[d]
    # the fp32 kernels' dynamic LDS: d = 380 sits just under 48 KB, d = 384 and d = 512 need the raised limit
    assert (4 * 32 * ((d + 3) // 4 * 4 + 1) > 48 * 1024) == (d >= 384)


def later_tiles(c, events, k):
    """per wavefront without a query node (no program's home) and with more than K0 columns: the events of the tiles behind the fill"""
    K0 = ts.k0_of(k)
    out = []
    for key, seq in ts.wave_columns(c["n"], c["cps"]).items():
        if key not in c["home"] and len(seq) > K0:
            assert all(e["full"] for e in events[key][K0 // 32:]) and not events[key][K0 // 32 - 1]["full"]
            out.append(events[key][K0 // 32:])
    assert len(out) >= 4 * (c["splits"] - 1) - c["P"]  # (all but the homes and a short last split)
    return out


@pytest.mark.parametrize("n,d,k", CASES)
def test_model_equals_the_reference_and_the_programs_drive_their_paths(n, d, k):
    c = ts.case(n, d, k)
    ev = {}
    for u in c["ids"][:c["P"] + 1].tolist():   # the query nodes and an ordinary node
        col, score, ev[u] = ts.model_topk(c["S"][u], c["cps"], k)
        want = ts.ref_topk(c["S"][u], k)
        assert np.array_equal(col, want[0]) and ts.bits_equal(score, want[1]), u
    q, P = c["q"], c["P"]
    blocks = (k - 1) // 64  # 64-entry register boundaries inside the list
    for tiles in later_tiles(c, ev[q["asc"]], k):
        for e in tiles:      # 32 entrants at the head (a partial last tile: fewer), everything else moves down by as many
            assert e["pos"] == list(range(min(e["cands"], k))) and e["shift"] == (e["cands"] if k > e["cands"] else 0) and e["cands"] == e["passed"]
            assert e["cands"] == 32 or e is tiles[-1]
            assert e["moved"] >= max(blocks, blocks * e["cands"] - 32)  # (at k > 64 entries cross every boundary)
        assert sum(e["cands"] == 32 for e in tiles) >= (2 if n == ts.N_LONG else 1)
    for tiles in later_tiles(c, ev[q["tail"]], k):
        assert all(e["pos"] == [k - 1] and e["passed"] == 1 and e["shift"] == 0 for e in tiles)
    for tiles in later_tiles(c, ev[q["head"]], k):
        assert all(e["pos"] == [0] and e["shift"] == min(1, k - 1) and e["moved"] == blocks for e in tiles)
    # the homed programs: the whole answer is the final list of ONE wavefront, which opens with the query node itself
    waves, K0 = ts.wave_columns(n, c["cps"]), ts.k0_of(k)
    for name in ts.HOMED:
        if name in q:
            home = c["home"][c["prog"][name]]
            assert set(ts.ref_topk(c["S"][q[name]], k)[0].tolist()) <= set(waves[home].tolist()), name
            tiles = ev[q[name]][home][K0 // 32:]
            assert len(tiles) >= 1 and all(e["full"] for e in tiles)
            if k > 1 and name == "tail":
                assert all(e["pos"] == [k - 1] and e["shift"] == 0 for e in tiles)
            if k > 1 and name == "head":
                assert all(e["pos"] == [1] and e["shift"] == 1 and e["moved"] == blocks for e in tiles)
            if k > 1 and name == "asc":
                assert all(e["pos"] == list(range(1, 1 + min(e["cands"], k - 1))) and e["shift"] == (e["cands"] if k > e["cands"] + 1 else 0) for e in tiles)
    if "const" in q:
        for tiles in later_tiles(c, ev[q["const"]], k):
            assert all(e["passed"] == e["cands"] > 0 and not e["pos"] for e in tiles)
        for tiles in later_tiles(c, ev[q["desc"]], k):
            assert all(e["passed"] == 0 for e in tiles)
        assert ts.totals(ev[q["desc"]])["full_insertions"] == 0
        t = ts.totals(ev[q["perm"]])
        assert t["full_insertions"] >= 2 * c["splits"] and (t["moved_between_blocks"] > 0 or k <= 64)
    # plateau: more than k columns share the k-th score, in several splits; lists are skipped in the merge and lists are merged
    if k == 1:
        return  # (the best column of every row is the query node itself)
    s = c["S"][q["plateau"]]
    kth = ts.ref_topk(s, k)[1][-1]
    members = np.flatnonzero(s == kth)
    assert kth == (ts.PLATEAU_KTH if k > 101 else ts.PLATEAU_TOP) and (s > kth).sum() < k < (s >= kth).sum()
    assert len(set((members // c["cps"]).tolist())) > c["splits"] // 2 and len(set(((members % c["cps"] % 128) // 32).tolist())) == 4
    m = ev[q["plateau"]]["merge"]
    assert m["merged"] > 4
    if "desc" in q:   # the merge skips every list whose head does not beat the running k-th key: all of the later splits but the homes
        assert ev[q["desc"]]["merge"]["skipped"] >= len(waves) - 4 - P
    tot = ts.totals(ev[q["plateau"]])
    assert tot["passed_nothing_entered"] > 0 or tot["full_insertions"] > 0


@pytest.mark.parametrize("k", ts.KS_LONG)
def test_long_case_at_every_k(k):
    """the long table is programmed for k = 256; at the other k the same rows still fill every list and insert into it"""
    c = ts.case(ts.N_LONG, ts.D_LONG, ts.K_LONG)
    splits, cps = ts.topk_plan(ts.N_LONG, ts.N_ROWS, k)
    for name in ("asc", "perm", "plateau", "head"):
        u = c["q"][name]
        col, score, ev = ts.model_topk(c["S"][u], cps, k)
        want = ts.ref_topk(c["S"][u], k)
        assert np.array_equal(col, want[0]) and ts.bits_equal(score, want[1]) and np.array_equal(want[0], ts.ref_topk(c["S"][u], 256)[0][:k])
        t = ts.totals(ev)
        assert t["full_insertions"] >= 4 * splits, (name, t)
        if name == "asc":
            assert t["largest_shift"] == (32 if k > 32 else 0) and (t["moved_between_blocks"] > 0) == (k > 64)


@pytest.mark.parametrize("k", ts.EXCLUDE_KS)
def test_exclusion_mixes_eligible_and_excluded_candidates_on_a_full_list(k):
    c = ts.case(ts.N_LONG, ts.D_LONG, k)
    n, cps = c["n"], c["cps"]
    nb = ts.neighbour_sets(n, ts.exclusion_edges(c))
    for name in ("asc", "plateau"):
        u = c["q"][name]
        elig = ts.eligibility(n, u, nb[u])
        col, score, ev = ts.model_topk(c["S"][u], cps, k, elig)
        want = ts.ref_topk(c["S"][u], k, elig)
        assert np.array_equal(col, want[0]) and ts.bits_equal(score, want[1]) and -1 not in col
        assert not np.array_equal(col, ts.ref_topk(c["S"][u], k)[0])  # the exclusion changes the answer
        mixed = sum(1 for key, tiles in ev.items() if key != "merge" for e in tiles if e["full"] and 0 < e["cands"] < e["passed"])
        assert mixed >= (4 if name == "asc" else 1), (name, mixed)
    assert len(nb[c["q"]["asc"]]) == min(600, c["cps"] // 4) // 2 and len(nb[c["q"]["plateau"]]) == 200
