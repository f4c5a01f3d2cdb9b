"""Hyper-parameters of the GraphGAN trainer.

Same names, meaning and defaults as the reference's flag module (``src/GraphGAN/config.py:1-41``)
so that a user's existing ``config.py`` keeps working: ``graph_gan.py`` here imports a module
called ``config`` from the working directory first and falls back to this file.  Knobs that only
exist for the MI355X engine are prefixed ``engine_`` and default to reference behaviour.
"""
import os

modes = ["gen", "dis"]  # order of emb_filenames / results lines

# ---- training (reference config.py:4-16)
batch_size_gen = 64
batch_size_dis = 64
lambda_gen = 1e-5
lambda_dis = 1e-5
n_sample_gen = 20
lr_gen = 1e-3
lr_dis = 1e-3
n_epochs = 20
n_epochs_gen = 30
n_epochs_dis = 30
gen_interval = n_epochs_gen
dis_interval = n_epochs_dis
update_ratio = 1

# ---- model saving (reference config.py:19-20)
load_model = False
save_steps = 10

# ---- other hyper-parameters (reference config.py:23-25)
n_emb = 50
multi_processing = False  # kept for compatibility; the C++ tree builder is always threaded
window_size = 2

# ---- application / dataset / paths (reference config.py:28-41), relative to the working directory
app = "link_prediction"
dataset = "CA-GrQc"
_base = os.environ.get("GRAPHGAN_ROOT", "../..")
train_filename = _base + "/data/" + app + "/" + dataset + "_train.txt"
test_filename = _base + "/data/" + app + "/" + dataset + "_test.txt"
test_neg_filename = _base + "/data/" + app + "/" + dataset + "_test_neg.txt"
labels_filename = _base + "/data/" + app + "/" + dataset + "_labels.txt"  # app = "node_classification": lines of "node label"
pretrain_emb_filename_d = _base + "/pre_train/" + app + "/" + dataset + "_pre_train.emb"
pretrain_emb_filename_g = _base + "/pre_train/" + app + "/" + dataset + "_pre_train.emb"
emb_filenames = [_base + "/results/" + app + "/" + dataset + "_gen_.emb",
                 _base + "/results/" + app + "/" + dataset + "_dis_.emb"]
result_filename = _base + "/results/" + app + "/" + dataset + ".txt"
cache_filename = _base + "/cache/" + dataset + ".pkl"
model_log = _base + "/log/"

# ---- engine-only knobs (no reference counterpart)
engine_seed = 0               # Philox key of the walk sampler + host RNG of root selection / batch shuffles
engine_optimizer = "adam_dense"  # "adam_dense" = TF1.8 semantics (parity); "adam_lazy" | "sgd" = scale modes
engine_device = 0
engine_tree_device = True    # BFS trees on the GPU (False: threaded host BFS, same trees)
engine_tree_threads = 0       # host BFS only; 0 = all host cores
engine_profile_every = 1      # HIP events on every k-th walk launch; 1 = every launch and pass (passes synchronous); 0 = none
engine_tree_budget_gb = 160.0  # all N BFS trees stay resident (reference :31-46) when they fit this much HBM; otherwise the epoch runs over root batches (gg_epoch_*)
engine_batch_roots = 0        # roots per batch of a root-batched epoch; 0 = what the budget holds (at most 16 384)
engine_emb_text = True        # write the reference's .emb text after every epoch (graph_gan.py:293-306); ~50 GB per write at N = 10^7, d = 256
engine_emb_sidecar = False    # also write <emb_filename>.bin: the same fp32 numbers in binary (utils.read_embeddings_bin)
engine_rec_ks = (2, 10, 20)   # app = "recommendation": the K of the P@K / R@K results line (each in [1, 256])
engine_rec_precision = "fp32"  # app = "recommendation": ranking scores in exact "fp32" or "bf16" (matrix-core bf16 inputs)
engine_gen_nll = False        # evaluation(): append "gen_nll:NLL=<nll> reach=<reach> n=<n>" -- the held-out NLL of the generator's graph softmax
# app = "node_classification": softmax regression on the frozen embeddings, fitted on the device (gg_classifier_fit).  The split
# seed is engine_seed.  The three fit defaults are provisional: they have not been measured on a labelled dataset.
engine_nc_train_ratio = 0.9   # share of the labelled nodes that trains the classifier (the paper's 9:1 split)
engine_nc_iters = 200         # full-batch Adam steps
engine_nc_lr = 0.05
engine_nc_l2 = 1e-4
# multi-label files (BlogCatalog, Wikipedia: lines of "node label [label ...]", utils.read_multilabels): one-vs-rest logistic
# regression on the device (gg_classifier_ml_fit) and the line "acc= micro_f1= macro_f1= n_train= n_test=".  Protocol "topk"
# predicts for a test node as many labels as it truly has (the customary protocol: it reads the test nodes' label COUNTS),
# "threshold" the classes with a positive logit.
engine_nc_multilabel = False
engine_nc_ml_protocol = "topk"
# learned link prediction (evaluation/link_prediction_lr.py): with engine_lp_classifier = True evaluation() appends, after the
# app's own lines, "gen_lp:acc= macro_f1= auc= n_train= n_test=" and "dis_lp:..." -- logistic regression on an operator of the two
# endpoint rows, fitted on the device (gg_edge_classifier_fit) on the training edges and as many sampled non-edges.  Needs
# test_filename and test_neg_filename.  The fit defaults are provisional: they have not been tuned on any dataset.
engine_lp_classifier = False
engine_lp_operator = "hadamard"  # "hadamard" | "average" | "l1" | "l2" (the node2vec paper's table)
engine_lp_iters = 200
engine_lp_lr = 0.05
engine_lp_l2 = 1e-4
engine_lp_max_train = 1 << 20    # training positives at most (a seeded subset beyond that)
# full-ranking link evaluation (evaluation/link_ranking.py): with engine_link_rank = True evaluation() appends, after the *_lp lines
# and before gen_nll, "gen_rank:MRR= MR= H@1= H@10= H@100= n=" and "dis_rank:..." -- the exact rank of every test edge (both
# directions) among all nodes but the source and its training neighbours, counted on the device (gg_rank_scores), filtered by the
# source's other test neighbours.  Needs test_filename; reads no negatives.
engine_link_rank = False
engine_link_rank_ks = (1, 10, 100)   # the K of H@K: any positive integers
engine_link_rank_precision = "fp32"  # ranking scores in exact "fp32" or "bf16" (matrix-core bf16 inputs)
# node clustering (evaluation/node_clustering.py): with engine_node_clustering = True evaluation() appends, under any app, after the
# *_rank lines and before gen_nll, "gen_cluster:NMI= ARI= purity= inertia= k= n= iters= empty=" and "dis_cluster:..." -- k-means on
# the frozen rows of ALL labelled nodes, seeded (k-means++) and fitted on the device (gg_kmeans_step / gg_kmeans_fit), scored against
# the labels.  Needs labels_filename (lines of "node label"); the restart seeds are engine_seed, engine_seed + 1, ...  The last two
# defaults are provisional: they have not been tuned on any dataset.
engine_node_clustering = False
engine_cluster_k = 0            # clusters; 0 = the number of distinct labels
engine_cluster_n_init = 4       # k-means++ restarts; the lowest final inertia is kept
engine_cluster_max_iters = 100  # Lloyd sweeps of a restart at most
# silhouette of those partitions (evaluation/node_silhouette.py): with engine_cluster_silhouette = True (needs engine_node_clustering)
# evaluation() appends, after the two *_cluster lines and before gen_nll, "gen_sil:sil= label_sil= k= n= rows= precision=" and
# "dis_sil:..." -- the exact mean silhouette over ALL pairs (gg_silhouette) of the k-means partition the *_cluster line reports and of
# the labels taken as the partition.  No labels are needed to COMPUTE a silhouette (Engine.silhouette); this evaluator reports both.
engine_cluster_silhouette = False
engine_sil_precision = "fp32"   # distances from exact "fp32" scores or "bf16" (the silhouette of the bf16-rounded table)
engine_sil_max_rows = 0         # 0 = every row; else a sample of that many rows (RandomState([engine_seed, 0x5349])) against all columns
# spectrum of the embedding rows (evaluation/embedding_spectrum.py): with engine_emb_spectrum = True evaluation() appends, under any
# app, after the *_sil lines and before gen_nll, "gen_spec:erank= pr= top1= top10= var= mean_norm= n= d=" and "dis_spec:..." -- the
# effective rank, participation ratio and leading shares of the covariance spectrum of the rows of the nodes with a training edge,
# their total variance and the norm of their mean (two gg_gram sweeps on the device, eigh on the host).  Needs no file beyond the
# training edges: no labels, no test edges, no negatives.
engine_emb_spectrum = False
# k-NN node classification (evaluation/node_knn.py): with engine_nc_knn = True evaluation() appends, under any app, after the *_spec
# lines and before gen_nll, "gen_knn:acc= macro_f1= k= metric= n_train= n_test=" and "dis_knn:..." -- every test node of the
# classifier's split (engine_nc_train_ratio, engine_seed) takes the majority label of its k nearest TRAINING nodes, found by one
# streamed top-K over that candidate set on the device (gg_topk_metric).  No optimiser, nothing to tune but k and the metric.
# Needs labels_filename (lines of "node label"); k may not exceed the number of training nodes.
engine_nc_knn = False
engine_knn_k = 10               # neighbours that vote, 1 .. 256
engine_knn_metric = "cosine"    # "cosine" | "l2" | "dot"
engine_knn_precision = "fp32"   # neighbour scores in exact "fp32" or "bf16" (matrix-core bf16 inputs)
# global top-K pair prediction (evaluation/pair_prediction.py): ONE ranking over all pairs {u, v}, u < v, of the nodes with a training
# edge by E[u] . E[v] (gg_top_pairs: a floor consumer on the tile stream; one call at max(engine_pair_ks) per line).  Both knobs work
# under any app and write one line per mode after the *_knn lines and before graph_lp; no negatives file is read.
#   engine_pair_prediction        "gen_pairs:P@<K>= R@<K>= ... n_test= dropped= n= found= precision=": the training edges are dropped
#                                 from the ranking; are the best-scored non-edges the held-out edges?  Needs test_filename.  Positives:
#                                 the distinct undirected test edges with both ends among those nodes that are no training edges or
#                                 self-loops; dropped counts the other test edges.
#   engine_graph_reconstruction   "gen_recon:P@<K>= R@<K>= ... edges= n= found= precision=": nothing is dropped; are the best-scored
#                                 pairs the training edges (SDNE / HOPE precision@K)?
# P@K = hits in the first min(K, found) entries / K, R@K = hits / positives.  The K are provisional: they have not been chosen on any dataset.
engine_pair_prediction = False
engine_graph_reconstruction = False
engine_pair_ks = (100, 1000, 10000)  # positive integers <= 2^20
engine_pair_precision = "fp32"       # pair scores in exact "fp32" or "bf16" (matrix-core bf16 inputs)
# neighbourhood link-prediction baselines (evaluation/link_heuristics.py): with engine_lp_heuristics = True evaluation() appends, under
# any app, after the *_knn lines and before gen_nll, ONE line "graph_lp:cn= jaccard= aa= ra= pa= n_test=" -- the AUC of common
# neighbours, Jaccard, Adamic-Adar, resource allocation and preferential attachment on the TRAINING graph over the test edges and
# test negatives (one pair-neighbour sweep on the device, gg_pair_neighbors).  No embedding takes part, so the line is computed at
# the first evaluation and repeated at every later one: the floor the *_lp lines stand on.  Needs test_filename and test_neg_filename.
engine_lp_heuristics = False
# label-spreading baseline of node classification (evaluation/label_propagation.py): with engine_nc_graph_baseline = True evaluation()
# appends, under any app, after the graph_lp line and before gen_nll, ONE line "graph_nc:acc= macro_f1= alpha= iters= delta= unreached=
# n_train= n_test=" (with engine_nc_multilabel: "acc= micro_f1= macro_f1= ...", protocol "topk" only) -- F <- alpha S F + (1 - alpha) Y on the
# TRAINING graph from the training labels of the classifier's split (engine_nc_train_ratio, engine_seed), iterated on the device
# (gg_label_spread).  No embedding takes part, so the line is computed at the first evaluation and repeated at every later one: what
# the graph and the labels alone predict.  Needs labels_filename.  Both defaults are provisional: they have not been tuned on any dataset.
engine_nc_graph_baseline = False
engine_lsp_alpha = 0.9          # in (0, 1): the share a node takes from its neighbours
engine_lsp_iters = 30           # iterations (a label travels one hop per iteration)
# label-propagation community baseline of node clustering (evaluation/graph_communities.py): with engine_cluster_graph_baseline = True
# evaluation() appends, under any app, after the graph_nc line and before gen_nll, ONE line "graph_cluster:NMI= ARI= purity= Q=
# communities= n= iters= converged= seed=" -- label-propagation communities of the WHOLE training graph, detected on the device
# (gg_label_propagation), the restart with the highest modularity Q kept (seeds engine_seed, engine_seed + 1, ...; the first on ties),
# scored against the labels over the labelled nodes.  No embedding takes part, so the line is computed at the first evaluation and
# repeated at every later one: what a community detector on the adjacency lists alone reaches.  Needs labels_filename.  Both defaults
# are provisional: they have not been tuned on any dataset.
engine_cluster_graph_baseline = False
engine_lpa_n_init = 4           # restarts; the highest modularity is kept
engine_lpa_max_iters = 100      # iterations of a restart at most (it stops at the first one that moves no label)
# modularity of the clustering lines' partitions (evaluation/graph_communities.py): with engine_cluster_modularity = True (needs
# engine_node_clustering) evaluation() appends, after the *_sil lines (after the *_cluster lines where there are none), "gen_mod:Q=
# label_Q= k= n= edges=" and "dis_mod:..." -- Newman's modularity, on the subgraph of the training graph that the labelled nodes induce,
# of the k-means partition the *_cluster line reports and of the labels taken as the partition (gg_partition_edges): whether the
# clusters of the embedding are communities of the graph.
engine_cluster_modularity = False
# graph-only ranking baselines (evaluation/graph_ranking.py): what ranking every node by a neighbourhood index on the training graph
# alone -- the two-hop sweep, gg_two_hop_rank / gg_two_hop_topk; no embedding takes part -- reaches on the two ranking evaluators.  Both
# knobs work under any app, need test_filename, and write one line per index of engine_graph_rank_indices, after the graph_cluster line
# and before gen_nll; the lines are computed at the first evaluation and repeated at every later one.
#   engine_link_rank_graph_baseline   "graph_rank:index=<i> MRR= MR= H@<K>= ... n= reach=": the queries, the filter and the K
#                                     (engine_link_rank_ks) of the *_rank lines; reach: the share of queries whose target scores > 0
#   engine_rec_graph_baseline         "graph_rec:index=<i> P@<K>= R@<K>= ...": the queries, the scoring and the K (engine_rec_ks) of
#                                     the app = "recommendation" lines
engine_link_rank_graph_baseline = False
engine_rec_graph_baseline = False
engine_graph_rank_indices = ("cn", "aa", "ra")   # common neighbours, Adamic-Adar, resource allocation
# rooted (personalised) PageRank as a further graph-only ranking baseline (evaluation/graph_ppr.py): the push sweep, gg_ppr_rank /
# gg_ppr_topk -- the local push of Andersen, Chung & Lang in fixed-point integers, which looks past the two hops of the indices above.
# Both knobs work under any app, need test_filename and write ONE line, computed at the first evaluation and repeated at every later one:
#   engine_link_rank_ppr_baseline   "graph_rank:index=ppr MRR= MR= H@<K>= ... n= reach= alpha= eps= rounds= converged= residual=" behind
#                                   the last graph_rank line (or where it would stand): rounds = the largest of any query, converged =
#                                   the share of queries whose push ended before engine_ppr_max_rounds, residual = the mean mass not pushed
#   engine_rec_ppr_baseline         "graph_rec:index=ppr P@<K>= R@<K>= ... alpha= eps=" behind the last graph_rec line
# The three parameters are untuned: the customary restart probability, and a threshold that keeps a query's work below 2^40 / kmin =
# 66 669 adjacency entries; they have been run on no dataset but the CA-GrQc fixture.
engine_link_rank_ppr_baseline = False
engine_rec_ppr_baseline = False
engine_ppr_alpha = 0.15         # restart probability, quantised to 2^-16
engine_ppr_eps = 1e-4           # push threshold per unit of degree, quantised to 2^-40 of the mass
engine_ppr_max_rounds = 200     # synchronous rounds of a query at most
# graph-only global top-K pair baseline (evaluation/graph_pairs.py): what "the K pairs with the largest neighbourhood index" on the
# training graph alone -- the two-hop pair sweep, gg_two_hop_top_pairs; no embedding takes part -- reach on the two protocols of the
# *_pairs / *_recon lines, with their node set, positives and K (engine_pair_ks).  Both knobs work under any app and write one line
# per index of engine_graph_rank_indices, behind the last graph_rec line (or where it would stand) and before gen_nll; the lines are
# computed at the first evaluation and repeated at every later one.
#   engine_pair_graph_baseline    "graph_pairs:index=<i> P@<K>= R@<K>= ... n_test= dropped= n= found=": the training edges are dropped
#                                 from the ranking.  Needs test_filename.
#   engine_recon_graph_baseline   "graph_recon:index=<i> P@<K>= R@<K>= ... edges= n= found=": nothing is dropped.
engine_pair_graph_baseline = False
engine_recon_graph_baseline = False
# skip-gram pre-training from uniform or node2vec (p, q) random walks (graphgan_amd/pretrain.py): with engine_pretrain = True a missing
# pretrain_emb_filename_* is produced on the device and written in the reference's .emb text before it is read
engine_pretrain = False
engine_pretrain_walks = 10    # walks per start node and epoch
engine_pretrain_len = 40      # nodes per walk
engine_pretrain_window = 5
engine_pretrain_neg = 5       # negatives per pair, drawn in proportion to round(16 * max(deg, 1) ^ 0.75)
engine_pretrain_epochs = 1
engine_pretrain_batch = 4096  # rows per optimizer step
engine_pretrain_lr = 5e-3
engine_pretrain_p = 1.0       # node2vec return parameter p and in-out parameter q, each in [1/16, 16] (pretrain.walk_bias);
engine_pretrain_q = 1.0       # p = q = 1 is the uniform (DeepWalk) walk
engine_pretrain_rows_per_call = 1 << 26  # rows one gg_prepare_pretrain call may produce (12 B each, device resident)
