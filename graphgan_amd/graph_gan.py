"""GraphGAN trainer: the reference's entry point (``src/GraphGAN/graph_gan.py``) on the MI355X engine.

Same class, method names, return shapes, schedule, file formats and ``config`` names as the
reference; every ``tf.Session.run`` call site and the interpreted walk sampler are replaced by
calls into ``libgraphgan_hip.so`` (``graphgan_amd.engine.Engine``):

    reference                                             here
    ----------------------------------------------------  -------------------------------------------
    utils.read_edges (utils.py:12-54)                     read_edges_csr (native ingest, same list order)
    construct_trees (:84-108) + pickle cache (:31-46)     Engine.build_trees (BFS on the GPU, or threaded host BFS)
    sample (:225-270) incl. sess.run(all_score) (:238)    Engine.walk_sample / prepare_d / prepare_g (K1)
    get_node_pairs_from_path (:272-291)                   device kernel inside prepare_g (K6)
    sess.run(discriminator.reward) (:220-222)             device kernel inside prepare_g (K2)
    sess.run(d_updates) loop (:149-157)                   Engine.d_pass (K3 + K5)
    sess.run(g_updates) loop (:168-176)                   Engine.g_pass (K4 + K5)
    sess.run(embedding_matrix) (:298) + text formatting   Engine.get_embeddings / write_embeddings (native, same bytes)
    tf.train.Saver (:55,124-127,137-138)                  Engine.save_state / load_state

Run exactly like the reference: ``cd src/GraphGAN && python <this file>`` -- a ``config.py`` in
the working directory (the reference's own) is honoured; otherwise ``graphgan_amd/config.py``.
Randomness: the reference draws from the unseeded global numpy RNG (Q5); here the walk sampler
uses Philox keyed by ``config.engine_seed`` and the host decisions (root selection, batch order)
use ``numpy.random.RandomState(engine_seed)``, so runs are reproducible.
"""
import math
import os
import sys
import time

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if __package__ in (None, ""):  # executed as a script: make the package importable
    sys.path.insert(0, os.path.dirname(_HERE))

try:  # the user's flag module in the working directory wins, as with the reference (graph_gan.py:8)
    if os.path.isfile(os.path.join(os.getcwd(), "config.py")) and os.getcwd() != _HERE:
        sys.path.insert(0, os.getcwd())
        import config  # noqa: E402
    else:
        raise ImportError
except ImportError:
    from graphgan_amd import config  # noqa: E402

from graphgan_amd import _lib, engine as _engine, parallel, utils  # noqa: E402
from graphgan_amd.evaluation import link_prediction as lp  # noqa: E402
from graphgan_amd.evaluation import link_prediction_lr as lplr  # noqa: E402
from graphgan_amd.evaluation import link_ranking as lrank  # noqa: E402
from graphgan_amd.evaluation import generator_likelihood as gl  # noqa: E402
from graphgan_amd.evaluation import recommendation as rec  # noqa: E402
from graphgan_amd.evaluation import node_classification as nc  # noqa: E402
from graphgan_amd.evaluation import node_clustering as ncl  # noqa: E402
from graphgan_amd.evaluation import node_silhouette as nsil  # noqa: E402
from graphgan_amd.evaluation import embedding_spectrum as espec  # noqa: E402
from graphgan_amd.evaluation import node_knn as nknn  # noqa: E402
from graphgan_amd.evaluation import pair_prediction as ppair  # noqa: E402
from graphgan_amd.evaluation import link_heuristics as lheur  # noqa: E402
from graphgan_amd.evaluation import label_propagation as lprop  # noqa: E402
from graphgan_amd.evaluation import graph_communities as gcomm  # noqa: E402
from graphgan_amd.evaluation import graph_ranking as grank  # noqa: E402
from graphgan_amd.evaluation import graph_ppr as gppr  # noqa: E402
from graphgan_amd.evaluation import graph_pairs as gpairs  # noqa: E402

_OPTIMIZERS = {"adam_dense": _lib.GG_OPT_ADAM_DENSE, "adam_lazy": _lib.GG_OPT_ADAM_LAZY, "sgd": _lib.GG_OPT_SGD}


def _cfg(cfg, name, default):
    return getattr(cfg, name, default)


def _check_gen_nll(cfg):
    """app = "node_classification" runs without test edges; the held-out NLL line does not (checked before anything is computed)"""
    if cfg.app == "node_classification" and _cfg(cfg, "engine_gen_nll", False) and not os.path.isfile(cfg.test_filename):
        raise ValueError("engine_gen_nll needs test edges: config.test_filename does not exist under app = 'node_classification'")


def _check_lp_classifier(cfg):
    """the learned link-prediction lines need both test files, under any app (checked before anything is computed)"""
    if not _cfg(cfg, "engine_lp_classifier", False):
        return
    for name in ("test_filename", "test_neg_filename"):
        path = getattr(cfg, name, None)
        if not path or not os.path.isfile(path):
            raise ValueError("engine_lp_classifier needs test edges and test negatives: config.%s does not exist (%r)" % (name, path))


def _check_lp_heuristics(cfg):
    """the neighbourhood baseline line needs both test files, under any app (checked before anything is computed)"""
    if not _cfg(cfg, "engine_lp_heuristics", False):
        return
    for name in ("test_filename", "test_neg_filename"):
        path = getattr(cfg, name, None)
        if not path or not os.path.isfile(path):
            raise ValueError("engine_lp_heuristics needs test edges and test negatives: config.%s does not exist (%r)" % (name, path))


def _check_nc_graph_baseline(cfg):
    """the label-spreading line needs the labels file, under any app, a share in (0, 1) and at least one iteration; multi-label
    files are scored by the "topk" protocol only (checked before anything is computed)"""
    if not _cfg(cfg, "engine_nc_graph_baseline", False):
        return
    path = getattr(cfg, "labels_filename", None)
    if not path or not os.path.isfile(path):
        raise ValueError("engine_nc_graph_baseline needs labels: config.labels_filename does not exist (%r)" % (path,))
    alpha, iters = _cfg(cfg, "engine_lsp_alpha", 0.9), _cfg(cfg, "engine_lsp_iters", 30)
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 < float(alpha) < 1.0:
        raise ValueError("engine_lsp_alpha must lie in (0, 1), got %r" % (alpha,))
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
        raise ValueError("engine_lsp_iters must be an integer >= 1, got %r" % (iters,))
    if _cfg(cfg, "engine_nc_multilabel", False) and _cfg(cfg, "engine_nc_ml_protocol", "topk") != "topk":
        raise ValueError("engine_nc_graph_baseline scores multi-label files by the 'topk' protocol only, got engine_nc_ml_protocol = %r"
                         % (_cfg(cfg, "engine_nc_ml_protocol", "topk"),))


def _check_cluster_graph_baseline(cfg):
    """the label-propagation community line needs the labels file, under any app, at least one restart and one iteration (checked
    before anything is computed)"""
    if not _cfg(cfg, "engine_cluster_graph_baseline", False):
        return
    path = getattr(cfg, "labels_filename", None)
    if not path or not os.path.isfile(path):
        raise ValueError("engine_cluster_graph_baseline needs labels: config.labels_filename does not exist (%r)" % (path,))
    for name, default in (("engine_lpa_n_init", 4), ("engine_lpa_max_iters", 100)):
        value = _cfg(cfg, name, default)
        if isinstance(value, bool) or not isinstance(value, int) or value < 1:
            raise ValueError("%s must be an integer >= 1, got %r" % (name, value))


def _check_graph_ranking(cfg):
    """the graph-only ranking lines need the test edges, under any app, known indices and the K of their evaluators (checked before
    anything is computed)"""
    for knob, ks_name, ks_default, cls in (("engine_link_rank_graph_baseline", "engine_link_rank_ks", lrank.DEFAULT_KS, grank.GraphRankEval),
                                           ("engine_rec_graph_baseline", "engine_rec_ks", (2, 10, 20), grank.GraphRecEval)):
        if not _cfg(cfg, knob, False):
            continue
        path = getattr(cfg, "test_filename", None)
        if not path or not os.path.isfile(path):
            raise ValueError("%s needs test edges: config.test_filename does not exist (%r)" % (knob, path))
        cls(cfg.train_filename, path, 1, indices=_cfg(cfg, "engine_graph_rank_indices", grank.INDICES), ks=tuple(_cfg(cfg, ks_name, ks_default)))


def _ppr_kw(cfg):
    return dict(alpha=_cfg(cfg, "engine_ppr_alpha", gppr.DEFAULT_ALPHA), eps=_cfg(cfg, "engine_ppr_eps", gppr.DEFAULT_EPS),
                max_rounds=_cfg(cfg, "engine_ppr_max_rounds", gppr.DEFAULT_MAX_ROUNDS))


def _check_graph_ppr(cfg):
    """the rooted-PageRank lines need the test edges, under any app, parameters inside the rule's ranges and the K of their evaluators
    (checked before anything is computed)"""
    for knob, ks_name, ks_default, cls in (("engine_link_rank_ppr_baseline", "engine_link_rank_ks", lrank.DEFAULT_KS, gppr.GraphPprRankEval),
                                           ("engine_rec_ppr_baseline", "engine_rec_ks", (2, 10, 20), gppr.GraphPprRecEval)):
        if not _cfg(cfg, knob, False):
            continue
        path = getattr(cfg, "test_filename", None)
        if not path or not os.path.isfile(path):
            raise ValueError("%s needs test edges: config.test_filename does not exist (%r)" % (knob, path))
        cls(cfg.train_filename, path, 1, ks=tuple(_cfg(cfg, ks_name, ks_default)), **_ppr_kw(cfg))


def _check_graph_pairs(cfg):
    """the graph-only pair lines need the training edges, graph_pairs also the test edges, under any app, known indices and the K of
    the pair lines (checked before anything is computed)"""
    pairs, recon = _cfg(cfg, "engine_pair_graph_baseline", False), _cfg(cfg, "engine_recon_graph_baseline", False)
    if not pairs and not recon:
        return
    name = "engine_pair_graph_baseline" if pairs else "engine_recon_graph_baseline"
    path = getattr(cfg, "train_filename", None)
    if not path or not os.path.isfile(path):
        raise ValueError("%s needs the training edges: config.train_filename does not exist (%r)" % (name, path))
    if pairs:
        path = getattr(cfg, "test_filename", None)
        if not path or not os.path.isfile(path):
            raise ValueError("engine_pair_graph_baseline needs test edges: config.test_filename does not exist (%r)" % (path,))
    grank.check_indices(_cfg(cfg, "engine_graph_rank_indices", grank.INDICES))
    ppair.check_ks(_cfg(cfg, "engine_pair_ks", ppair.DEFAULT_KS))


def _check_link_rank(cfg):
    """the full-ranking lines need the test edges, under any app (checked before anything is computed)"""
    if not _cfg(cfg, "engine_link_rank", False):
        return
    path = getattr(cfg, "test_filename", None)
    if not path or not os.path.isfile(path):
        raise ValueError("engine_link_rank needs test edges: config.test_filename does not exist (%r)" % (path,))


def _check_node_clustering(cfg):
    """the clustering lines need the labels file, under any app (checked before anything is computed); the silhouette lines
    judge the clustering lines' partition"""
    if _cfg(cfg, "engine_cluster_silhouette", False) and not _cfg(cfg, "engine_node_clustering", False):
        raise ValueError("engine_cluster_silhouette needs engine_node_clustering = True: it scores the k-means partition of the *_cluster lines")
    if _cfg(cfg, "engine_cluster_modularity", False) and not _cfg(cfg, "engine_node_clustering", False):
        raise ValueError("engine_cluster_modularity needs engine_node_clustering = True: it scores the k-means partition of the *_cluster lines")
    if not _cfg(cfg, "engine_node_clustering", False):
        return
    path = getattr(cfg, "labels_filename", None)
    if not path or not os.path.isfile(path):
        raise ValueError("engine_node_clustering needs labels: config.labels_filename does not exist (%r)" % (path,))


def _check_emb_spectrum(cfg):
    """the spectrum lines need two nodes with a training edge, under any app (checked before anything is computed)"""
    if not _cfg(cfg, "engine_emb_spectrum", False):
        return
    path = getattr(cfg, "train_filename", None)
    if not path or not os.path.isfile(path):
        raise ValueError("engine_emb_spectrum needs the training edges: config.train_filename does not exist (%r)" % (path,))
    n = len(espec.trained_nodes(path))
    if n < 2:
        raise ValueError("engine_emb_spectrum needs at least two nodes with a training edge: %r has %d" % (path, n))


def _check_pair_prediction(cfg):
    """the pair lines need the training edges, gen_pairs also the test edges, under any app (checked before anything is computed)"""
    pairs, recon = _cfg(cfg, "engine_pair_prediction", False), _cfg(cfg, "engine_graph_reconstruction", False)
    if not pairs and not recon:
        return
    name = "engine_pair_prediction" if pairs else "engine_graph_reconstruction"
    path = getattr(cfg, "train_filename", None)
    if not path or not os.path.isfile(path):
        raise ValueError("%s needs the training edges: config.train_filename does not exist (%r)" % (name, path))
    if pairs:
        path = getattr(cfg, "test_filename", None)
        if not path or not os.path.isfile(path):
            raise ValueError("engine_pair_prediction needs test edges: config.test_filename does not exist (%r)" % (path,))
    ppair.check_ks(_cfg(cfg, "engine_pair_ks", ppair.DEFAULT_KS))
    ppair.check_precision(_cfg(cfg, "engine_pair_precision", "fp32"))


def _check_node_knn(cfg):
    """the k-NN lines need the labels file, under any app, and at most as many neighbours as the split has training nodes (checked
    before anything is computed)"""
    if not _cfg(cfg, "engine_nc_knn", False):
        return
    path = getattr(cfg, "labels_filename", None)
    if not path or not os.path.isfile(path):
        raise ValueError("engine_nc_knn needs labels: config.labels_filename does not exist (%r)" % (path,))
    metric = _cfg(cfg, "engine_knn_metric", "cosine")
    if metric not in nknn.METRICS:
        raise ValueError("engine_knn_metric must be 'dot', 'cosine' or 'l2', got %r" % (metric,))
    with open(path, "r") as f:
        n_labelled = sum(1 for line in f if line.split())  # (utils.read_labels: one node per non-blank line)
    n_train = int(math.ceil(float(_cfg(cfg, "engine_nc_train_ratio", 0.9)) * n_labelled))
    nknn.check_k(_cfg(cfg, "engine_knn_k", 10), n_train)


class GraphGAN(object):
    def __init__(self, cfg=None):
        self.config = cfg if cfg is not None else config
        cfg = self.config
        print("reading graphs...")
        # native ingest (same adjacency as utils.read_edges, utils.py:12-47); self.graph[i] still lists i's neighbours
        _check_gen_nll(cfg)
        _check_lp_classifier(cfg)
        _check_link_rank(cfg)
        _check_node_clustering(cfg)
        _check_emb_spectrum(cfg)
        _check_node_knn(cfg)
        _check_pair_prediction(cfg)
        _check_lp_heuristics(cfg)
        _check_nc_graph_baseline(cfg)
        _check_cluster_graph_baseline(cfg)
        _check_graph_ranking(cfg)
        test_filename = cfg.test_filename
        if cfg.app == "node_classification" and not os.path.isfile(test_filename):
            test_filename = ""  # the app has no test edges
        self.n_node, self._rowptr, self._col = _engine.read_edges_csr(cfg.train_filename, test_filename)
        self.graph = _engine.CSRGraph(self._rowptr, self._col)
        # One process per GPU (torch.distributed.run exports RANK / WORLD_SIZE / LOCAL_RANK; a plain `python graph_gan.py`
        # is world 1).  The reference is a single tf.Session (:57-61): every rank here holds full replicas of both models,
        # walks ITS share of the roots (:188, :208 -- the walk RNG is keyed by root id, so the share does not change a
        # walk) and the replicas sum their gradients inside every optimizer step (:154, :173; RCCL inside the engine).
        self.ctl = parallel.Control()
        self.rank, self.world = self.ctl.rank, self.ctl.world
        self.all_root_nodes = [i for i in range(self.n_node)]
        deg = (self._rowptr[1:] - self._rowptr[:-1]).astype(np.int64)
        # degree-balanced shares (D-mode walks per root = its degree); world 1: all roots, in id order like the reference
        self.root_nodes = [int(r) for r in parallel.shard_roots(np.arange(self.n_node), self.rank, self.world,
                                                                weights=deg if self.world > 1 else None)]
        self._prepare_no = 0
        self._graph_lp_line = None  # the graph_lp results line (engine_lp_heuristics): a function of the files alone, computed once
        self._graph_nc_line = None  # the graph_nc results line (engine_nc_graph_baseline) likewise
        self._graph_cluster_line = None  # the graph_cluster results line (engine_cluster_graph_baseline) likewise
        self._graph_rank_lines = None  # the graph_rank / graph_rec results lines (engine_link_rank_graph_baseline, engine_rec_graph_baseline) likewise
        self._graph_rec_lines = None
        self._graph_pairs_lines = None  # the graph_pairs / graph_recon results lines (engine_pair_graph_baseline, engine_recon_graph_baseline) likewise
        self._graph_recon_lines = None

        self.seed = int(_cfg(cfg, "engine_seed", 0))
        # rows missing from the pre-trained file are drawn from the global numpy RNG (utils.py:63); the
        # reference never seeds it (Q5) -- seeding it here makes the whole run reproducible
        np.random.seed(self.seed)
        # engine_pretrain: a missing pre-trained file is produced from the edge list (skip-gram on uniform or node2vec --
        # engine_pretrain_p / _q -- random walks, on the device) and written in the reference's .emb text; the unchanged read below then finds it.  Off by default: a missing
        # file raises as in the reference.  With replicas rank 0 writes, the others wait for the file.
        if _cfg(cfg, "engine_pretrain", False):
            from graphgan_amd import pretrain as _pretrain
            if self.rank == 0:
                _pretrain.ensure_pretrained(cfg, self.n_node, self._rowptr, self._col)
            self.ctl.barrier()
        print("reading initial embeddings...")
        self.node_embed_init_d = utils.read_embeddings(filename=cfg.pretrain_emb_filename_d, n_node=self.n_node,
                                                       n_embed=cfg.n_emb)
        self.node_embed_init_g = utils.read_embeddings(filename=cfg.pretrain_emb_filename_g, n_node=self.n_node,
                                                       n_embed=cfg.n_emb)

        self.host_rng = np.random.RandomState(self.seed if self.world == 1 else [self.seed, self.rank])

        print("building GAN model...")
        self.engine = None
        self.generator = None
        self.discriminator = None
        self.build_generator()
        self.build_discriminator()

        # BFS trees live in HBM; like the reference's self.trees (:31-46) every root stays resident for the whole
        # run -- also with update_ratio < 1, where each prepare call only SELECTS a subset of the resident slots, so
        # the in-place D-mode mutations (Q3, :258-259) persist across epochs exactly as in the reference.  When all N
        # trees cannot fit the budget (config.engine_tree_budget_gb; N^2 storage: 12 TB at 10^6 nodes) the epoch runs
        # over ROOT BATCHES instead (_prepare_root_batches / gg_epoch_*): the same schedule -- prepare over all (selected)
        # roots, then the passes over all rows -- with one batch of trees resident at a time and the mutation bits kept
        # in a store that outlives the trees.
        print("constructing BFS-trees...")
        self.trees = None
        self._slot_of_root = None
        self._all_resident = False
        self._g_pairs_ready = False
        budget = float(_cfg(cfg, "engine_tree_budget_gb", 160.0)) * 2.0 ** 30
        # roots per batch of a root-batched epoch (all N trees do not fit: N^2 storage): what the budget holds
        self._batch_roots = int(_cfg(cfg, "engine_batch_roots", 0)) or max(1, min(16384, int(budget // self.engine.tree_bytes_estimate(1))))
        if self.engine.tree_bytes_estimate(len(self.root_nodes)) <= budget:
            # construct or read BFS-trees (reference :31-46; the cache is a flat GGTR file instead of a pickle)
            cache = self._tree_cache_path(_cfg(cfg, "cache_filename", None))
            if cache and os.path.isfile(cache) and self._load_tree_cache(cache):
                print("reading BFS-trees from cache...")
            else:
                self.trees = self.construct_trees(self.root_nodes)
                # the reference needs `mkdir cache` too (README.md:43); a file of another format is never overwritten
                if cache and os.path.isdir(os.path.dirname(cache) or ".") and self._is_ours_or_absent(cache):
                    self.engine.save_trees(cache)
            self._all_resident = True

        self.latest_checkpoint = os.path.join(cfg.model_log, "model.checkpoint.ggst")

    # ------------------------------------------------------------------ model construction
    def _ensure_engine(self):
        if self.engine is None:
            cfg = self.config
            self.engine = _engine.Engine(
                self.node_embed_init_g, self.node_embed_init_d, lr_gen=cfg.lr_gen, lr_dis=cfg.lr_dis,
                lambda_gen=cfg.lambda_gen, lambda_dis=cfg.lambda_dis, window_size=cfg.window_size,
                optimizer=_OPTIMIZERS[_cfg(cfg, "engine_optimizer", "adam_dense")],
                device=int(_cfg(cfg, "engine_device", 0)) if self.world == 1 else self.ctl.local_rank)
            if int(_cfg(cfg, "engine_profile_every", 1)) != 1:
                self.engine.set_profiling(int(_cfg(cfg, "engine_profile_every", 1)))
            self.engine.set_graph_csr(self._rowptr, self._col)
            self.ctl.connect_engine(self.engine)  # world > 1: RCCL communicator (unique id over the gloo control plane)
        return self.engine

    def build_generator(self):
        """initializing the generator (table [n_node, n_emb] from the pre-trained rows, zero bias)"""
        self._ensure_engine()
        self.generator = _ModelView(self.engine, 0)

    def build_discriminator(self):
        """initializing the discriminator"""
        self._ensure_engine()
        self.discriminator = _ModelView(self.engine, 1)

    def construct_trees(self, nodes):
        """BFS trees of ``nodes`` (reference :84-108) -> resident tree CSR; returns the slot map
        root -> slot (the reference returns the dict of dicts itself)."""
        nodes = np.asarray(list(nodes), dtype=np.int32)
        self.engine.build_trees(nodes, n_threads=int(_cfg(self.config, "engine_tree_threads", 0)),
                                device=bool(_cfg(self.config, "engine_tree_device", True)))
        self._slot_of_root = {int(r): i for i, r in enumerate(nodes)}
        return self._slot_of_root

    def _tree_cache_path(self, name):
        """File of the native tree cache for ``config.cache_filename``.  The reference pickles to that very name
        (``cache/<dataset>.pkl``, :36-46); a pickle found there is neither readable by gg_load_trees nor ours to replace, so
        the flat GGTR cache lives NEXT to it: ``<name>.ggtr`` (per rank with replicas: every rank caches its own roots)."""
        if not name:
            return None
        path = name if name.endswith(".ggtr") else name + ".ggtr"
        if self.world > 1:
            path = "%s.rank%dof%d" % (path, self.rank, self.world)
        return path

    @staticmethod
    def _is_ours_or_absent(path):
        if not os.path.exists(path):
            return True
        try:
            with open(path, "rb") as f:
                return f.read(4) == b"GGTR"
        except OSError:
            return False

    def _load_tree_cache(self, path):
        """Resident trees from the cache file if it holds exactly the trees of ``root_nodes`` for this graph."""
        try:
            self.engine.load_trees(path)
        except _lib.GraphGANHipError as e:  # foreign / stale / truncated file: rebuild (and overwrite) instead of failing
            print("tree cache %s not used: %s" % (path, e))
            return False
        roots = np.asarray(self.engine.tree_roots)
        if len(roots) != len(self.root_nodes) or not np.array_equal(roots, np.asarray(self.root_nodes, dtype=np.int32)):
            print("tree cache %s holds other roots: rebuilding" % path)
            return False
        self._slot_of_root = {int(r): i for i, r in enumerate(roots)}
        self.trees = self._slot_of_root
        return True

    def construct_trees_with_mp(self, nodes):
        """kept for API compatibility (reference :63-82): the C++ builder is always multi-threaded"""
        self.trees = self.construct_trees(nodes)

    # ------------------------------------------------------------------ training
    @staticmethod
    def stream_id(epoch, inner_epoch, n_inner, for_d):
        """Philox stream of a prepare call: distinct per (outer epoch, inner epoch, phase)."""
        return 2 * (epoch * max(n_inner, 1) + inner_epoch) + (0 if for_d else 1)

    def train(self):
        cfg = self.config
        if os.path.isfile(self.latest_checkpoint) and cfg.load_model:
            print("loading the checkpoint: %s" % self.latest_checkpoint)
            self.engine.load_state(self.latest_checkpoint)

        if self.rank == 0:  # the replicas are identical: one of them writes
            self.write_embeddings_to_file()
            self.evaluation(self)

        print("start training...")
        for epoch in range(cfg.n_epochs):
            print("epoch %d" % epoch)

            if epoch > 0 and epoch % cfg.save_steps == 0 and self.rank == 0:
                os.makedirs(cfg.model_log, exist_ok=True)
                self.engine.save_state(self.latest_checkpoint)

            # D-steps
            t_epoch = time.time()
            train_size = 0
            self._g_pairs_ready = False
            for d_epoch in range(cfg.n_epochs_dis):
                if d_epoch % cfg.dis_interval == 0:
                    self._stream = self.stream_id(epoch, d_epoch, cfg.n_epochs_dis, True)
                    if self._all_resident:
                        train_size = self._prepare_d_resident()
                    else:
                        # the G-mode walks of the epoch's first generator prepare read the generator, the trees and the Q3 bits
                        # only (reference :204-216) -- nothing the remaining D passes change: they share the trees of the LAST
                        # discriminator prepare of the epoch (one BFS per root and outer epoch instead of two).  With
                        # update_ratio < 1 the two prepares draw their own roots (:189, :209): no sharing.
                        last = d_epoch + cfg.dis_interval >= cfg.n_epochs_dis
                        g_too = last and cfg.n_epochs_gen > 0 and cfg.update_ratio >= 1
                        train_size = self._prepare_root_batches(True, g_too, self._stream, self.stream_id(epoch, 0, cfg.n_epochs_gen, False))
                        self._g_pairs_ready = g_too
                if self._all_resident and d_epoch == cfg.n_epochs_dis - 1 and cfg.n_epochs_gen > 0 and cfg.update_ratio >= 1:
                    # the G-mode walks of the first G epoch read the generator only (reference :204-216): started on the
                    # engine's side stream before the last D pass is enqueued, adopted by prepare_g below (same arguments; with
                    # update_ratio < 1 the root draw of that call is not known yet, and nothing is begun)
                    self.engine.prepare_g_begin(self._select_slots(), cfg.n_sample_gen, self.seed, self.stream_id(epoch, 0, cfg.n_epochs_gen, False))
                self.engine.d_pass(self._batch_starts(train_size, cfg.batch_size_dis), cfg.batch_size_dis)

            # G-steps
            train_size = 0
            for g_epoch in range(cfg.n_epochs_gen):
                if g_epoch % cfg.gen_interval == 0:
                    self._stream = self.stream_id(epoch, g_epoch, cfg.n_epochs_gen, False)
                    if self._all_resident:
                        train_size = self._prepare_g_resident()
                    elif g_epoch == 0 and self._g_pairs_ready:
                        train_size = self.engine.epoch_commit(0)  # pairs sampled beside the last D prepare; rewards evaluated now
                        self._g_pairs_ready = False
                    else:
                        train_size = self._prepare_root_batches(False, True, 0, self._stream)
                self.engine.g_pass(self._batch_starts(train_size, cfg.batch_size_gen), cfg.batch_size_gen)

            if self.rank == 0:
                self.write_embeddings_to_file()
                results = self.evaluation(self)
                self._write_perf_log(epoch, time.time() - t_epoch, results)
        print("training completes")

    def _batch_starts(self, train_size, batch_size):
        """One inner epoch's minibatches (reference :149-152, :168-171): the shuffled list of contiguous batch starts over
        THIS rank's prepared rows.  With replicas, step k of the pass is the union of every rank's k-th batch (a global
        batch of up to world * batch_size rows whose gradients the engine sums); ranks with fewer batches pad their list
        with -1 = "nothing from me in this step", so that all ranks issue the same number of steps (each step is a
        collective)."""
        start_list = list(range(0, train_size, batch_size))
        self.host_rng.shuffle(start_list)
        if self.world > 1:
            n_steps = int(self.ctl.max(len(start_list)))
            start_list += [-1] * (n_steps - len(start_list))
        return start_list

    # ------------------------------------------------------------------ sample preparation
    def _draw_roots(self):
        """``np.random.rand() < update_ratio`` per root (reference :189, :209): one draw per root, in root order
        (no draws with update_ratio >= 1: every root is taken, and the oracle trainer does the same).  Returns indices
        into ``root_nodes``."""
        cfg = self.config
        if cfg.update_ratio >= 1:
            return np.arange(len(self.root_nodes), dtype=np.int32)
        self._prepare_no += 1
        if self.world == 1:
            take = np.flatnonzero(self.host_rng.rand(len(self.root_nodes)) < cfg.update_ratio)
        else:  # one draw per ROOT of the whole graph, keyed by the prepare call: the selection does not depend on the sharding
            draws = np.random.RandomState([self.seed, self._prepare_no]).rand(self.n_node)
            take = np.flatnonzero(draws[np.asarray(self.root_nodes, dtype=np.int64)] < cfg.update_ratio)
        return take.astype(np.int32)

    def _select_slots(self):
        """The resident slots of this prepare call's roots (slot i holds root_nodes[i])."""
        assert self._all_resident
        return self._draw_roots()

    def _prepare_root_batches(self, do_d, do_g, stream_d, stream_g):
        """prepare_data_for_d and / or prepare_data_for_g (reference :182-223) over this call's roots when their trees
        cannot all be resident: batch by batch (gg_epoch_add: BFS trees on the GPU, Q3 bits restored / saved, walks, rows
        and pairs appended in root order), then the discriminator rows -- or, for a generator-only call, the pairs -- become
        the prepared data of the passes.  A rank that drew no root still commits (the call holds the replicas' collective)."""
        cfg = self.config
        roots = np.asarray(self.root_nodes, dtype=np.int32)[self._draw_roots()]
        self.engine.epoch_begin(reset_d=do_d, reset_g=do_g)
        for k in range(0, len(roots), self._batch_roots):
            self.engine.epoch_add(roots[k:k + self._batch_roots], do_d, do_g, cfg.n_sample_gen, self.seed, stream_d, stream_g)
        self._slot_of_root = None  # (the resident slots are the last batch's)
        return self.engine.epoch_commit(1 if do_d else 0)

    # An empty draw (update_ratio < 1) still goes through the engine: gg_prepare_* ends with a collective over the replicas
    # (the max of the ranks' row counts) that every rank must join, and it resets the resident row count that the passes and
    # their row-pack capacity read -- skipping the call left stale rows behind and, with world > 1, the other ranks waiting.
    def _prepare_d_resident(self):
        slots = self._select_slots()
        return self.engine.prepare_d(slots, self.seed, self._stream, fetch=False)

    def _prepare_g_resident(self):
        slots = self._select_slots()
        return self.engine.prepare_g(slots, self.config.n_sample_gen, self.seed, self._stream, fetch=False)

    def prepare_data_for_d(self):
        """generate positive and negative samples for the discriminator (reference :182-202);
        returns (center_nodes, neighbor_nodes, labels) and leaves them resident for d_pass"""
        if not hasattr(self, "_stream"):
            self._stream = 0
        if not self._all_resident:
            self._prepare_root_batches(True, False, self._stream, 0)
            center, neighbor, label = self.engine.get_d_data()
            return center.tolist(), neighbor.tolist(), label.astype(np.int64).tolist()
        slots = self._select_slots()
        if len(slots) == 0:
            return [], [], []
        center, neighbor, label, _ = self.engine.prepare_d(slots, self.seed, self._stream)
        return center.tolist(), neighbor.tolist(), label.astype(np.int64).tolist()

    def prepare_data_for_g(self):
        """sample nodes for the generator (reference :204-223); returns (node_1, node_2, reward)"""
        if not hasattr(self, "_stream"):
            self._stream = 1
        if not self._all_resident:
            self._prepare_root_batches(False, True, 0, self._stream)
            n1, n2, reward = self.engine.get_g_data()
            return n1.tolist(), n2.tolist(), reward
        slots = self._select_slots()
        if len(slots) == 0:
            return [], [], np.zeros(0, dtype=np.float32)
        n1, n2, reward, _ = self.engine.prepare_g(slots, self.config.n_sample_gen, self.seed, self._stream)
        return n1.tolist(), n2.tolist(), reward

    def sample(self, root, tree, sample_num, for_d):
        """sample nodes from the BFS-tree of ``root`` (reference :225-270).  ``tree`` is accepted
        for signature compatibility; the resident tree of ``root`` is used.
        Returns (samples, paths), or (None, None) when the reference would."""
        if self._slot_of_root is None or int(root) not in self._slot_of_root:
            if self._all_resident:
                raise KeyError("root %d has no resident tree (not in root_nodes)" % int(root))
            self.trees = self.construct_trees([int(root)])  # on-demand mode: build this root's tree
        slot = self._slot_of_root[int(root)]
        stream = getattr(self, "_stream", 0)
        res = self.engine.walk_sample([slot], [sample_num], for_d, self.seed, stream)
        if res["root_status"][0] == _lib.GG_ROOT_ABORTED:
            return None, None
        paths = [res["paths"][j, : res["path_len"][j]].tolist() for j in range(sample_num)]
        return res["samples"].tolist(), paths

    @staticmethod
    def get_node_pairs_from_path(path):
        """window pairs of a path whose last element (the back-step) is dropped (reference :272-291);
        host twin of the device kernel, kept for API compatibility"""
        window = config.window_size
        nodes = path[:-1]
        pairs = []
        for i, center in enumerate(nodes):
            lo, hi = max(i - window, 0), min(i + window + 1, len(nodes))
            pairs.extend([center, nodes[j]] for j in range(lo, hi) if j != i)
        return pairs

    # ------------------------------------------------------------------ outputs
    def write_embeddings_to_file(self):
        """write embeddings of the generator and the discriminator to files (reference :293-306):
        header ``N<TAB>d``, then ``id<TAB>v0<TAB>...``; values are the fp32 numbers widened to
        fp64 and printed with ``str`` (what ``np.hstack([index, matrix]).tolist()`` gives)"""
        cfg = self.config
        for i in range(2):
            os.makedirs(os.path.dirname(cfg.emb_filenames[i]) or ".", exist_ok=True)
            if _cfg(cfg, "engine_emb_text", True):
                self.engine.write_embeddings(i, cfg.emb_filenames[i])  # native formatter, byte-identical text
            if _cfg(cfg, "engine_emb_sidecar", False):
                self.engine.write_embeddings_bin(i, cfg.emb_filenames[i] + ".bin")  # same numbers, 4 B each

    def _write_perf_log(self, epoch, wall_s, results):
        """One JSON line per outer epoch beside the results file (``<result_filename>.perf.jsonl``): wall time, the engine's
        counters (walks, sampled edges, rows scored, pairs through the passes, optimizer steps, tree builds) and the
        accuracies just appended to the results file (reference :316-319 writes only those)."""
        import json
        cfg = self.config
        c = self.engine.counters()
        prev = getattr(self, "_perf_prev", {})
        delta = {k: c[k] - prev.get(k, 0) for k in ("walks", "hops", "rows_scored", "d_pairs", "g_pairs", "d_steps", "g_steps", "bfs_trees", "bfs_kernel_ms", "walk_reruns")}
        self._perf_prev = c
        rec = {"epoch": int(epoch), "wall_s": wall_s, "sampled_edges_per_sec": delta["hops"] / wall_s if wall_s > 0 else None,
               "trees": "resident" if self._all_resident else "root batches of %d" % self._batch_roots, "world": self.world,
               "results": [r.strip() for r in (results or [])], **delta}
        os.makedirs(os.path.dirname(cfg.result_filename) or ".", exist_ok=True)
        with open(cfg.result_filename + ".perf.jsonl", "a") as f:
            f.write(json.dumps(rec) + "\n")

    def gen_likelihood(self):
        """dict(nll, reach, n): every test edge in both directions under the G-mode distribution of its first node
        (evaluation/generator_likelihood.py).  Resident trees: the resident slots and their Q3 bits; root batches: whole trees
        built for batches of test roots with the Q3 bits of the epochs' store (the training's own trees are rebuilt by every
        epoch_add anyway)."""
        ev = gl.GenLikelihoodEval(self.config.test_filename, self.n_node, engine=self.engine,
                                  slot_of_root=self._slot_of_root if self._all_resident else None, batch_roots=self._batch_roots)
        return ev.eval_gen_likelihood()

    @staticmethod
    def evaluation(self):
        cfg = self.config
        _check_gen_nll(cfg)
        _check_lp_classifier(cfg)
        _check_link_rank(cfg)
        _check_node_clustering(cfg)
        _check_emb_spectrum(cfg)
        _check_node_knn(cfg)
        _check_pair_prediction(cfg)
        _check_lp_heuristics(cfg)
        _check_nc_graph_baseline(cfg)
        _check_cluster_graph_baseline(cfg)
        _check_graph_ranking(cfg)
        _check_graph_ppr(cfg)
        _check_graph_pairs(cfg)
        results = []
        if cfg.app == "link_prediction":
            for i in range(2):
                # the per-edge dots run on the device (gg_edge_scores) instead of re-reading the text just written
                lpe = lp.LinkPredictEval(cfg.emb_filenames[i], cfg.test_filename, cfg.test_neg_filename, self.n_node, cfg.n_emb,
                                         engine=self.engine, which=i)
                result = lpe.eval_link_prediction()
                results.append(cfg.modes[i] + ":" + str(result) + "\n")
        elif cfg.app == "recommendation":
            # P@K / R@K of a streamed top-K on the device (gg_topk_scores, exclude = the training graph); one line per mode:
            # "gen:P@2=<p> R@2=<r> P@10=... R@10=... P@20=... R@20=..." (no test-negatives file is read)
            ks = tuple(_cfg(cfg, "engine_rec_ks", (2, 10, 20)))
            for i in range(2):
                re_ = rec.RecommendEval(cfg.emb_filenames[i], cfg.train_filename, cfg.test_filename, self.n_node, cfg.n_emb,
                                        engine=self.engine, which=i, ks=ks, precision=_cfg(cfg, "engine_rec_precision", "fp32"))
                results.append(rec.format_results(cfg.modes[i], re_.eval_recommendation(), ks))
        elif cfg.app == "node_classification":
            # accuracy / Macro-F1 of softmax regression on the frozen rows, fitted and applied on the device (gg_classifier_*); one
            # line per mode: "gen:acc=<a> macro_f1=<f> n_train=<n> n_test=<n>".  With engine_nc_multilabel: one-vs-rest logistic
            # regression on "node label [label ...]" files (gg_classifier_ml_*), "gen:acc=<a> micro_f1=<f> macro_f1=<f> n_train= n_test="
            if not hasattr(cfg, "labels_filename"):
                raise ValueError("app = 'node_classification' needs config.labels_filename (lines of 'node label')")
            multilabel = bool(_cfg(cfg, "engine_nc_multilabel", False))
            for i in range(2):
                nce = nc.NodeClassifyEval(cfg.emb_filenames[i], cfg.labels_filename, self.n_node, cfg.n_emb, engine=self.engine, which=i,
                                          train_ratio=float(_cfg(cfg, "engine_nc_train_ratio", 0.9)), seed=self.seed,
                                          iters=int(_cfg(cfg, "engine_nc_iters", 200)), lr=float(_cfg(cfg, "engine_nc_lr", 0.05)),
                                          l2=float(_cfg(cfg, "engine_nc_l2", 1e-4)), multilabel=multilabel,
                                          ml_protocol=_cfg(cfg, "engine_nc_ml_protocol", "topk"))
                results.append((nc.format_ml_results if multilabel else nc.format_results)(cfg.modes[i], nce.eval_node_classification()))
        if _cfg(cfg, "engine_lp_classifier", False):
            # learned link prediction (gg_edge_classifier_*): logistic regression on an operator of the two endpoint rows, fitted on
            # training edges and sampled non-edges; one line per mode: "gen_lp:acc=<a> macro_f1=<f> auc=<u> n_train=<n> n_test=<n>"
            # (without an engine: the float64 host fit on the .emb text, as the other evaluators re-read it)
            for i in range(2):
                emd = None if self.engine is not None else utils.read_embeddings(cfg.emb_filenames[i], n_node=self.n_node, n_embed=cfg.n_emb)
                lre = lplr.LinkPredictLREval(cfg.train_filename, cfg.test_filename, cfg.test_neg_filename, self.n_node, cfg.n_emb,
                                             emd=emd, engine=self.engine, which=i, operator=_cfg(cfg, "engine_lp_operator", "hadamard"),
                                             iters=int(_cfg(cfg, "engine_lp_iters", 200)), lr=float(_cfg(cfg, "engine_lp_lr", 0.05)),
                                             l2=float(_cfg(cfg, "engine_lp_l2", 1e-4)), seed=self.seed,
                                             max_train=int(_cfg(cfg, "engine_lp_max_train", 1 << 20)))
                results.append(lplr.format_results(cfg.modes[i], lre.eval_link_prediction()))
        if _cfg(cfg, "engine_link_rank", False):
            # full ranking of the held-out edges (gg_rank_scores, exclude = the training graph; no negatives file): one line per
            # mode, "gen_rank:MRR=<m> MR=<r> H@1=<h> H@10=<h> H@100=<h> n=<n>" (without an engine: the float64 host ranking on the
            # .emb text)
            ks = tuple(_cfg(cfg, "engine_link_rank_ks", lrank.DEFAULT_KS))
            for i in range(2):
                lre = lrank.LinkRankEval(cfg.emb_filenames[i], cfg.train_filename, cfg.test_filename, self.n_node, cfg.n_emb,
                                         engine=self.engine, which=i, ks=ks, precision=_cfg(cfg, "engine_link_rank_precision", "fp32"))
                results.append(lrank.format_results(cfg.modes[i], lre.eval_link_ranking(), ks))
        if _cfg(cfg, "engine_node_clustering", False):
            # k-means on the frozen rows of all labelled nodes (gg_kmeans_step / gg_kmeans_fit), scored against the labels: one line
            # per mode, "gen_cluster:NMI=<n> ARI=<a> purity=<p> inertia=<i> k=<k> n=<n> iters=<t> empty=<e>" (without an engine: the
            # float64 host k-means on the .emb text)
            fits = []
            for i in range(2):
                nce = ncl.NodeClusterEval(cfg.emb_filenames[i], cfg.labels_filename, self.n_node, cfg.n_emb, engine=self.engine, which=i,
                                          k=int(_cfg(cfg, "engine_cluster_k", 0)), n_init=int(_cfg(cfg, "engine_cluster_n_init", 4)),
                                          max_iters=int(_cfg(cfg, "engine_cluster_max_iters", 100)), seed=self.seed)
                results.append(ncl.format_results(cfg.modes[i], nce.eval_node_clustering()))
                fits.append(nce.last_partition)
            if _cfg(cfg, "engine_cluster_silhouette", False):
                # exact silhouette over all pairs (gg_silhouette) of the partitions just reported and of the labels: one line per
                # mode, "gen_sil:sil=<s> label_sil=<l> k=<k> n=<n> rows=<r> precision=<p>" (without an engine: float64 on the .emb text)
                for i in range(2):
                    emd = None if self.engine is not None else utils.read_embeddings(cfg.emb_filenames[i], n_node=self.n_node, n_embed=cfg.n_emb)
                    nse = nsil.NodeSilhouetteEval(self.n_node, cfg.n_emb, engine=self.engine, emd=emd, which=i,
                                                  precision=_cfg(cfg, "engine_sil_precision", "fp32"),
                                                  max_rows=int(_cfg(cfg, "engine_sil_max_rows", 0)), seed=self.seed)
                    fit = fits[i]
                    results.append(nsil.format_results(cfg.modes[i], nse.eval_node_silhouette(fit["nodes"], fit["classes"], fit["assign"], fit["k"])))
            if _cfg(cfg, "engine_cluster_modularity", False):
                # modularity, on the subgraph of the training graph induced by the labelled nodes, of the partitions just reported and
                # of the labels (gg_partition_edges): one line per mode, "gen_mod:Q=<q> label_Q=<l> k=<k> n=<n> edges=<e>" (without an
                # engine: the same integers from numpy on the training file, the same string)
                if self.engine is not None:
                    edges = gcomm.engine_sweeps(self.engine)[1]
                else:
                    edges = gcomm.host_sweeps(utils.read_edges_from_file(cfg.train_filename), self.n_node)[1]
                for i in range(2):
                    results.append(gcomm.format_modularity(cfg.modes[i], gcomm.eval_cluster_modularity(edges, self.n_node, fits[i])))
        if _cfg(cfg, "engine_emb_spectrum", False):
            # spectrum of the covariance of the rows of the nodes with a training edge (two gg_gram sweeps, eigh on the host): one
            # line per mode, "gen_spec:erank=<e> pr=<p> top1=<t> top10=<t> var=<v> mean_norm=<n> n=<n> d=<d>" (without an engine: the
            # same two passes in float64 on the .emb text); no labels, test edges or negatives are read
            for i in range(2):
                ese = espec.EmbeddingSpectrumEval(cfg.emb_filenames[i], cfg.train_filename, self.n_node, cfg.n_emb, engine=self.engine, which=i)
                results.append(espec.format_results(cfg.modes[i], ese.eval_embedding_spectrum()))
        if _cfg(cfg, "engine_nc_knn", False):
            # k-NN classification of the test nodes of the classifier's split among its training nodes (one gg_topk_metric query
            # over that candidate set, the vote on the host): one line per mode, "gen_knn:acc=<a> macro_f1=<f> k=<k> metric=<m>
            # n_train=<n> n_test=<n>" (without an engine: the same definition in float64 on the .emb text)
            for i in range(2):
                emd = None if self.engine is not None else utils.read_embeddings(cfg.emb_filenames[i], n_node=self.n_node, n_embed=cfg.n_emb)
                nke = nknn.NodeKnnEval(cfg.labels_filename, self.n_node, cfg.n_emb, engine=self.engine, emd=emd, which=i,
                                       k=_cfg(cfg, "engine_knn_k", 10), metric=_cfg(cfg, "engine_knn_metric", "cosine"),
                                       precision=_cfg(cfg, "engine_knn_precision", "fp32"),
                                       train_ratio=float(_cfg(cfg, "engine_nc_train_ratio", 0.9)), seed=self.seed)
                results.append(nknn.format_results(cfg.modes[i], nke.eval_node_knn()))
        if _cfg(cfg, "engine_pair_prediction", False) or _cfg(cfg, "engine_graph_reconstruction", False):
            # the head of ONE ranking over all pairs of the nodes with a training edge (gg_top_pairs; one call at max(ks) per line):
            # "gen_pairs:P@<k>=<p> R@<k>=<r> ... n_test=<t> dropped=<d> n=<m> found=<f> precision=<p>" (the training edges dropped, the
            # held-out edges the positives), then "gen_recon:P@<k>=<p> R@<k>=<r> ... edges=<e> n=<m> found=<f> precision=<p>" (nothing
            # dropped, the training edges the positives); without an engine: float64 numpy on the .emb text
            ks = ppair.check_ks(_cfg(cfg, "engine_pair_ks", ppair.DEFAULT_KS))
            evs = []
            for i in range(2):
                emd = None if self.engine is not None else utils.read_embeddings(cfg.emb_filenames[i], n_node=self.n_node, n_embed=cfg.n_emb)
                evs.append(ppair.PairPredictionEval(cfg.train_filename, getattr(cfg, "test_filename", None), self.n_node, cfg.n_emb, engine=self.engine,
                                                    emd=emd, which=i, ks=ks, precision=_cfg(cfg, "engine_pair_precision", "fp32")))
            if _cfg(cfg, "engine_pair_prediction", False):
                for i in range(2):
                    results.append(ppair.format_pairs(cfg.modes[i], evs[i].eval_pair_prediction(), ks))
            if _cfg(cfg, "engine_graph_reconstruction", False):
                for i in range(2):
                    results.append(ppair.format_recon(cfg.modes[i], evs[i].eval_graph_reconstruction(), ks))
        if _cfg(cfg, "engine_lp_heuristics", False):
            # neighbourhood baselines on the training graph (gg_pair_neighbors): ONE line, "graph_lp:cn=<auc> jaccard=<auc> aa=<auc>
            # ra=<auc> pa=<auc> n_test=<n>" -- the graph is the same for both tables and every evaluation, so the line is computed
            # once and repeated (without an engine: the same integers from numpy on the training file, the same string)
            if getattr(self, "_graph_lp_line", None) is None:
                lhe = lheur.LinkHeuristicsEval(cfg.train_filename, cfg.test_filename, cfg.test_neg_filename, self.n_node, engine=self.engine)
                self._graph_lp_line = lheur.format_results(lhe.eval_link_heuristics())
            results.append(self._graph_lp_line)
        if _cfg(cfg, "engine_nc_graph_baseline", False):
            # label spreading on the training graph from the training labels of the classifier's split (gg_label_spread): ONE line,
            # "graph_nc:acc=<a> macro_f1=<f> alpha=<a> iters=<t> delta=<d> unreached=<u> n_train=<n> n_test=<n>" (multi-label: micro_f1
            # behind acc) -- computed once and repeated, like graph_lp (without an engine: float64 numpy on the training file)
            if getattr(self, "_graph_nc_line", None) is None:
                multilabel = bool(_cfg(cfg, "engine_nc_multilabel", False))
                lse = lprop.LabelSpreadEval(cfg.train_filename, cfg.labels_filename, self.n_node, engine=self.engine,
                                            train_ratio=float(_cfg(cfg, "engine_nc_train_ratio", 0.9)), seed=self.seed,
                                            alpha=float(_cfg(cfg, "engine_lsp_alpha", 0.9)), iters=int(_cfg(cfg, "engine_lsp_iters", 30)),
                                            multilabel=multilabel)
                self._graph_nc_line = lprop.format_results(lse.eval_label_spread(), multilabel)
            results.append(self._graph_nc_line)
        if _cfg(cfg, "engine_cluster_graph_baseline", False):
            # label-propagation communities of the whole training graph (gg_label_propagation), the restart with the highest
            # modularity, scored against the labels: ONE line, "graph_cluster:NMI=<n> ARI=<a> purity=<p> Q=<q> communities=<c> n=<n>
            # iters=<t> converged=<b> seed=<s>" -- computed once and repeated, like graph_lp (without an engine: numpy on the
            # training file, the same string)
            if getattr(self, "_graph_cluster_line", None) is None:
                gce = gcomm.GraphCommunityEval(cfg.train_filename, cfg.labels_filename, self.n_node, engine=self.engine,
                                               n_init=int(_cfg(cfg, "engine_lpa_n_init", 4)), max_iters=int(_cfg(cfg, "engine_lpa_max_iters", 100)),
                                               seed=self.seed)
                self._graph_cluster_line = gcomm.format_results(gce.eval_graph_communities())
            results.append(self._graph_cluster_line)
        # The ranking evaluators' graph-only lines, computed once and repeated, like graph_lp (without an engine: numpy on the training
        # file, the same strings).  Two-hop sweep (gg_two_hop_rank / gg_two_hop_topk): per index of engine_graph_rank_indices,
        # "graph_rank:index=<i> MRR=<m> MR=<r> H@1=<h> ... n=<n> reach=<r>" and "graph_rec:index=<i> P@2=<p> R@2=<r> ...".  Push sweep
        # (gg_ppr_rank / gg_ppr_topk): "graph_rank:index=ppr ... alpha=<a> eps=<e> rounds=<r> converged=<c> residual=<r>" behind the last
        # graph_rank line and "graph_rec:index=ppr ... alpha=<a> eps=<e>" behind the last graph_rec line, or where they would stand.
        kw = dict(engine=self.engine, indices=_cfg(cfg, "engine_graph_rank_indices", grank.INDICES))
        if _cfg(cfg, "engine_link_rank_graph_baseline", False):
            if getattr(self, "_graph_rank_lines", None) is None:
                self._graph_rank_lines = grank.GraphRankEval(cfg.train_filename, cfg.test_filename, self.n_node,
                                                             ks=tuple(_cfg(cfg, "engine_link_rank_ks", lrank.DEFAULT_KS)), **kw).lines()
            results.extend(self._graph_rank_lines)
        if _cfg(cfg, "engine_link_rank_ppr_baseline", False):
            if getattr(self, "_graph_ppr_rank_lines", None) is None:
                self._graph_ppr_rank_lines = gppr.GraphPprRankEval(cfg.train_filename, cfg.test_filename, self.n_node, engine=self.engine,
                                                                   ks=tuple(_cfg(cfg, "engine_link_rank_ks", lrank.DEFAULT_KS)), **_ppr_kw(cfg)).lines()
            results.extend(self._graph_ppr_rank_lines)
        if _cfg(cfg, "engine_rec_graph_baseline", False):
            if getattr(self, "_graph_rec_lines", None) is None:
                self._graph_rec_lines = grank.GraphRecEval(cfg.train_filename, cfg.test_filename, self.n_node,
                                                           ks=tuple(_cfg(cfg, "engine_rec_ks", (2, 10, 20))), **kw).lines()
            results.extend(self._graph_rec_lines)
        if _cfg(cfg, "engine_rec_ppr_baseline", False):
            if getattr(self, "_graph_ppr_rec_lines", None) is None:
                self._graph_ppr_rec_lines = gppr.GraphPprRecEval(cfg.train_filename, cfg.test_filename, self.n_node, engine=self.engine,
                                                                 ks=tuple(_cfg(cfg, "engine_rec_ks", (2, 10, 20))), **_ppr_kw(cfg)).lines()
            results.extend(self._graph_ppr_rec_lines)
        # The pair lines' graph-only lines (gg_two_hop_top_pairs: the two-hop pair sweep; one call at max(engine_pair_ks) per index and
        # line), computed once and repeated like the lines above: per index of engine_graph_rank_indices "graph_pairs:index=<i>
        # P@<k>=<p> R@<k>=<r> ... n_test=<t> dropped=<d> n=<m> found=<f>", then "graph_recon:index=<i> P@<k>=<p> R@<k>=<r> ... edges=<e>
        # n=<m> found=<f>" -- the node set, the positives and the scoring of the *_pairs / *_recon lines.
        if _cfg(cfg, "engine_pair_graph_baseline", False) or _cfg(cfg, "engine_recon_graph_baseline", False):
            gpe = gpairs.GraphPairsEval(cfg.train_filename, getattr(cfg, "test_filename", None), self.n_node, engine=self.engine,
                                        indices=_cfg(cfg, "engine_graph_rank_indices", grank.INDICES), ks=_cfg(cfg, "engine_pair_ks", ppair.DEFAULT_KS))
            if _cfg(cfg, "engine_pair_graph_baseline", False):
                if getattr(self, "_graph_pairs_lines", None) is None:
                    self._graph_pairs_lines = gpe.lines("pairs")
                results.extend(self._graph_pairs_lines)
            if _cfg(cfg, "engine_recon_graph_baseline", False):
                if getattr(self, "_graph_recon_lines", None) is None:
                    self._graph_recon_lines = gpe.lines("recon")
                results.extend(self._graph_recon_lines)
        if _cfg(cfg, "engine_gen_nll", False):
            # held-out NLL of the generator's graph softmax (gg_graph_softmax): "gen_nll:NLL=<nll> reach=<reach> n=<n>"
            results.append(gl.format_line(self.gen_likelihood()))
        os.makedirs(os.path.dirname(cfg.result_filename) or ".", exist_ok=True)
        with open(cfg.result_filename, mode="a+") as f:
            f.writelines(results)
        return results


class _ModelView(object):
    """Stand-in for the reference's Generator / Discriminator objects: exposes the variables the
    driver fetches (``embedding_matrix``, ``bias_vector``) as numpy arrays read from the engine."""

    def __init__(self, eng, which):
        self._eng, self._which = eng, which

    @property
    def embedding_matrix(self):
        return self._eng.get_embeddings(self._which)

    @property
    def bias_vector(self):
        return self._eng.get_bias(self._which)


if __name__ == "__main__":
    graph_gan = GraphGAN()
    graph_gan.train()
