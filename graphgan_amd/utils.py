"""Graph / embedding readers with the reference's semantics (``src/utils.py:12-67``).

Neighbour order matters downstream (it is the BFS child order and the order of the D-step
positives), so the adjacency lists keep file order exactly like the reference's dict of lists.
"""
import numpy as np


def read_edges_from_file(filename):
    """One edge per line, whitespace separated integer ids (utils.py:50-54)."""
    edges = []
    with open(filename, "r") as f:
        for line in f:
            edges.append([int(tok) for tok in line.split()])
    return edges


def read_edges(train_filename, test_filename):
    """-> (n_node, graph) with graph[v] = neighbours of v over the TRAIN edges in file order, both
    directions (a self-loop lists v twice); nodes that only occur in the test file get an empty
    list; n_node = number of distinct ids seen (utils.py:12-47)."""
    graph = {}
    train = read_edges_from_file(train_filename)
    test = read_edges_from_file(test_filename) if test_filename != "" else []
    for a, b in train:
        graph.setdefault(a, []).append(b)
        graph.setdefault(b, []).append(a)
    for a, b in test:
        graph.setdefault(a, [])
        graph.setdefault(b, [])
    return len(graph), graph


def read_labels(filename, n_node):
    """Lines of ``node<whitespace>label`` (integer labels of any value, one label per node; blank lines are skipped)
    -> (nodes int64 sorted, classes int64 in [0, C), label_values int64 [C] sorted): ``classes[i]`` is the rank of the label of
    ``nodes[i]`` among the distinct label values.  A node listed twice or an id outside [0, n_node) raises ValueError."""
    seen = {}
    with open(filename, "r") as f:
        for no, line in enumerate(f, 1):
            tok = line.split()
            if not tok:
                continue
            if len(tok) != 2:
                raise ValueError("%s:%d: expected 'node label', got %r" % (filename, no, line.strip()))
            node, label = int(tok[0]), int(tok[1])
            if not 0 <= node < n_node:
                raise ValueError("%s:%d: node id %d outside [0, %d)" % (filename, no, node, n_node))
            if node in seen:
                raise ValueError("%s:%d: node %d is listed twice (one label per node)" % (filename, no, node))
            seen[node] = label
    nodes = np.array(sorted(seen), dtype=np.int64)
    labels = np.array([seen[int(v)] for v in nodes], dtype=np.int64)
    values, classes = np.unique(labels, return_inverse=True)
    return nodes, classes.astype(np.int64).reshape(-1), values.astype(np.int64)


MAX_LABELS = 128  # the classifier's class limit (include/graphgan_hip.h, gg_classifier_*)


def read_multilabels(filename, n_node):
    """Lines of ``node label [label ...]`` (any whitespace, integer labels of any value; blank lines are skipped).  A node may
    appear on several lines: its labels are the union, a repeated (node, label) is harmless.
    -> (nodes int64 sorted, Y bool [L, C], label_values int64 [C] sorted): ``Y[i, c]`` says that ``nodes[i]`` has the label
    whose rank among the distinct label values is c.  An id outside [0, n_node), a line with fewer than two tokens or more than
    128 distinct labels raises ValueError."""
    seen = {}
    with open(filename, "r") as f:
        for no, line in enumerate(f, 1):
            tok = line.split()
            if not tok:
                continue
            if len(tok) < 2:
                raise ValueError("%s:%d: expected 'node label [label ...]', got %r" % (filename, no, line.strip()))
            node = int(tok[0])
            if not 0 <= node < n_node:
                raise ValueError("%s:%d: node id %d outside [0, %d)" % (filename, no, node, n_node))
            seen.setdefault(node, set()).update(int(t) for t in tok[1:])
    nodes = np.array(sorted(seen), dtype=np.int64)
    values = np.array(sorted(set().union(*seen.values())) if seen else [], dtype=np.int64)
    if len(values) > MAX_LABELS:
        raise ValueError("%s: %d distinct labels, the classifier takes at most %d" % (filename, len(values), MAX_LABELS))
    rank = {int(v): c for c, v in enumerate(values.tolist())}
    Y = np.zeros((len(nodes), len(values)), dtype=bool)
    for i, v in enumerate(nodes.tolist()):
        Y[i, [rank[x] for x in seen[v]]] = True
    return nodes, Y, values


def read_embeddings(filename, n_node, n_embed):
    """``.emb`` text -> float64 [n_node, n_embed]; the first line is a header; rows whose id is
    absent keep uniform [0, 1) draws from the global numpy RNG (utils.py:57-67)."""
    emb = np.random.rand(n_node, n_embed)
    with open(filename, "r") as f:
        f.readline()
        for line in f:
            tok = line.split()
            if tok:
                emb[int(tok[0]), :] = [float(x) for x in tok[1:]]
    return emb


def read_embeddings_bin(filename):
    """Binary side-car written next to the ``.emb`` text (``Engine.write_embeddings_bin``) -> float32 [n_node, n_emb]."""
    with open(filename, "rb") as f:
        head = f.read(20)
        if head[:4] != b"GGEB" or np.frombuffer(head, "<i4", 1, 4)[0] != 1:
            raise ValueError("%s is not a GGEB v1 file" % filename)
        n_emb = int(np.frombuffer(head, "<i4", 1, 8)[0])
        n_node = int(np.frombuffer(head, "<i8", 1, 12)[0])
        return np.fromfile(f, dtype="<f4", count=n_node * n_emb).reshape(n_node, n_emb)
