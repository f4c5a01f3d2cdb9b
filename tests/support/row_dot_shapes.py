"""What tests/test_gpu_walk_widths.py, the width tests of tests/test_gpu_graph_softmax.py and tests/test_gpu_steps.py, and
tests/test_row_dot_shapes_cpu.py share: a plain-Python restatement of how the training path picks a template instance of its
row dot from the row width, the case lists, and the tables.

The row dot (spec S1; oracle: orc_dot16).  A 16-lane group works on float4 chunks of a row of ld floats
(ld = n_emb rounded up to a multiple of 4): lane t owns chunks t, t + 16, ..., runs one fmaf chain over them, and an xor
butterfly combines the lanes.  The kernels are instantiated by the number of chunks a lane can own, nch = ceil(ld / 4 / 16):

    level_score_kernel<NCH>, walk_sample_kernel<NCH, LAZY> (walk_sample.hip, launch_walk_sample)  NCH = 1, 2, 4, 8
    gs_fill_kernel<NCH>                                     (graph_softmax.hip)                    NCH = 1, 2, 4, 8
    path_reward_kernel<NCH>                                 (prepare.hip, enqueue_g_pairs)         NCH = 1, 2, 4; declined
                                                             when nch > 4 or window > 2: the pairs are filled and
                                                             pair_reward_kernel runs on the device-side count
Above ld = 256 the staged gradient (steps.hip, staged_allowed) and the whole-walk generator pass (steps.hip, run_pass) are
declined as well.  tests/test_row_dot_shapes_cpu.py checks that the copied lines are still in the sources.

Tables.  table(n, d) draws rows randn * d^-1/4, so the score of two different nodes has standard deviation ~1 at every width
(a node's score with itself is ~sqrt(d)): the softmax of a candidate list is neither flat nor one-hot, and every 64-column
block of a row carries an equal share of a score -- zeroing one changes the walks (checked on the CPU)."""
import numpy as np

MAX_EMB = 512  # gg_create: n_emb > 512 is refused


def cdiv(a, b):
    return -(-a // b)


def ld_of(d):
    """the row stride of the resident tables: d rounded up to a multiple of 4"""
    return cdiv(d, 4) * 4


def nch_of(d):
    """float4 chunks per lane of a 16-lane group: const int nch = (a.nchunk + 15) / 16 with nchunk = ld / 4"""
    return cdiv(ld_of(d) // 4, 16)


def instance_of(d):
    """the template instance every four-way ladder picks: nch <= 1 / == 2 / <= 4 / <= 8"""
    nch = nch_of(d)
    assert 1 <= nch <= 8, "n_emb %d not supported (max %d)" % (d, MAX_EMB)
    return 1 if nch <= 1 else 2 if nch == 2 else 4 if nch <= 4 else 8


def path_reward_taken(d, window=2):
    """enqueue_g_pairs: the whole-walk reward kernel runs (ld % 4 == 0 always holds for the padded tables)"""
    return window <= 2 and nch_of(d) <= 4


def path_reward_instance(d, window=2):
    """the path_reward_kernel instance (nch <= 1 / == 2 / else), None where the kernel is declined"""
    if not path_reward_taken(d, window):
        return None
    nch = nch_of(d)
    return 1 if nch <= 1 else 2 if nch == 2 else 4


def wide(d):
    """ld > 256: no staged gradient, no whole-walk generator pass, no whole-walk reward"""
    return ld_of(d) > 256


# ---- case lists ----------------------------------------------------------------------------------------------------------------
# one chunk into the next instance: 65 (<2>: only lane 0 owns a second chunk), 129 (nch = 3 runs <4>), 257 (nch = 5 runs <8>);
# rows padded inside the last float4: 1, 509; the widest row: 512
WIDTHS = (1, 6, 64, 65, 128, 129, 192, 256, 257, 260, 320, 509, 512)
INSTANCE_WIDTHS = (6, 65, 129, 257, 512)  # one width per instance, <8> at its narrowest and at its widest

WALK_MODES = ("levels", "finisher", "hybrid2", "share_all", "share_off")
LAZY_MODES = ("levels", "finisher", "hybrid2")
FINISHER_SCORES = ("finisher", "hybrid2")  # modes in which walk_sample_kernel (through score_block) scores hops itself


def walk_env(mode):
    """the environment of tests/test_gpu_walk.py's walk_mode fixture (and of tests/test_gpu_lazy.py's) for these names; gg_create
    reads the variables, so they are set before the engine exists"""
    env = {"GG_WALK_LEVELS": {"finisher": "0", "hybrid2": "2"}.get(mode, "64")}
    if mode in ("share_all", "share_off"):
        env["GG_ES_MODE"] = "2" if mode == "share_all" else "0"
    return env


# walks on load_small(1): every instance in every mode, the other widths in the two modes that own a score kernel each
WALK_CASES = [(d, m) for d in INSTANCE_WIDTHS for m in WALK_MODES] + \
             [(d, m) for d in WIDTHS if d not in INSTANCE_WIDTHS for m in ("levels", "finisher")]
# the 1 501-candidate hub list at a wide row: score_block<8> with its HBM-scratch branch (finisher), the hub path of the levels
HUB_LEAVES, HUB_WIDTH = 1500, 320
HUB_CASES = [(HUB_WIDTH, "finisher"), (HUB_WIDTH, "levels")]
# lazy trees: (golden graph, node_cap) x width x mode; d = 6 keeps <1, lazy> in this matrix beside the wide instances
LAZY_GRAPHS = ((1, 8), (3, 8))
LAZY_WIDTHS = (6, 128, 256, 257, 512)
LAZY_CASES = [(gi, cap, d, m) for gi, cap in LAZY_GRAPHS for d in LAZY_WIDTHS for m in LAZY_MODES]
# graph softmax on load_small(3); d = 6 and d = 65 keep <1> and <2> in this list beside <4> and <8>
GS_WIDTHS = (6, 65, 129, 256, 257, 512)
# rewards of prepare_g on load_small(3); d = 6 keeps path_reward_kernel<1> in this list; 257 and 512 decline the kernel
REWARD_WIDTHS = (6, 65, 128, 129, 257, 512)
# prepare_d, d_pass, prepare_g, g_pass with SGD on load_small(3): the last width the staged and whole-walk paths accept, and two
# beyond it
PASS_WIDTHS = (256, 260, 512)


def table(n, d):
    """(rows fp32 [n, d], bias fp32 [n]) of width d"""
    rs = np.random.RandomState(d)
    E = (rs.randn(n, d) * d ** -0.25).astype(np.float32)
    b = (rs.randn(n) * 0.2).astype(np.float32)
    return E, b


# ---- the fp32 score error of the tables ------------------------------------------------------------------------------------------
# e(d) = max over the edges (u, v) of load_small(3) of |fp32 score - float64 score|, score = E[u] . E[v] + b[v] on table(90, d), the
# fp32 score from the oracle (c_all_score_rows on the padded table).  Measured by tests/test_row_dot_shapes_cpu.py, which fails
# when a value here is below what it measures or more than 1 % above it.
E_SCORE = {6: 2.569e-07, 65: 1.202e-06, 129: 3.170e-06, 256: 7.696e-06, 257: 4.471e-06, 512: 9.608e-06}


def logp_tolerance(d, max_depth, tol_logp):
    """The bound of a graph-softmax log-probability at width d where the file's own tol_logp does not hold: a log-probability
    sums at most max_depth + 1 hop terms, each carries the score error e(d) once in its numerator and at most once in its
    log-sum; the factor 2 is the margin for the fp32 softmax arithmetic."""
    return max(tol_logp, 2.0 * (max_depth + 2) * E_SCORE[d])
