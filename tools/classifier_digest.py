#!/usr/bin/env python3
"""SHA-256 over the raw bytes of every output of the six node-classification entry points (gg_classifier_lossgrad / _fit /
_predict and their multi-label forms), of gg_kmeans_step / _fit (with and without the sums, centroids by value and by node id)
and of the three gg_edge_classifier_* entry points for the four operators, on fixed inputs: the shapes of the device tests'
fits plus (997, 256, 128), whose second operand is staged in k-chunks, and (32769, 8, 2), which has more tiles than workgroups
(C is also k).  The paths are deterministic (no floating-point atomics), so two builds that compute the same thing print the
same list: run it in the tree of each build and compare.
    python tools/classifier_digest.py
One JSON line: {"digests": {"<entry point> (M, d, C)[ output]": "<sha256>", ...}, "all": "<sha256 of the list>"}."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import graphgan_amd as ga  # noqa: E402

SHAPES = [(997, 8, 5), (1500, 50, 7), (1500, 50, 33), (4099, 128, 40), (997, 256, 128), (32769, 8, 2)]
ITERS = 20

digests = {}


def put(call, shape, outputs):
    for name, a in outputs:
        digests["%s %r %s" % (call, shape, name)] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


for M, d, C in SHAPES:
    rs = np.random.RandomState(31 * M + d + C)
    table = (0.3 * rs.randn(M + 1000, d)).astype(np.float32)
    eng = ga.Engine(table, table[::-1].copy())
    nodes = rs.permutation(M + 1000)[:M]
    y = rs.randint(0, C, size=M)
    Y = np.zeros((M, C), dtype=bool)
    Y[np.arange(M), y] = True
    Y[np.arange(M), rs.randint(0, C, size=M)] = True  # one or two labels per row
    W = (0.5 * rs.randn(C, d)).astype(np.float32)
    b = (0.5 * rs.randn(C)).astype(np.float32)
    k = Y.sum(axis=1).astype(np.int32)
    cen = (0.3 * rs.randn(C, d)).astype(np.float32)  # (drawn behind everything the classifier calls use)
    v = rs.permutation(M + 1000)[:M]
    ye = rs.randint(0, 2, size=M)
    we, be = (0.5 * rs.randn(d)).astype(np.float32), float(np.float32(0.5 * rs.randn()))
    for which in (0, 1):
        shape = (M, d, C, which)
        for call, labels in (("classifier_lossgrad", y), ("classifier_ml_lossgrad", Y)):
            r = getattr(eng, call)(nodes, labels, W, b, which=which, l2=1e-3)
            put(call, shape, (("loss", np.float32(r["loss"])), ("gW", r["gW"]), ("gb", r["gb"])))
        for call, labels in (("classifier_fit", y), ("classifier_ml_fit", Y)):
            r = getattr(eng, call)(nodes, labels, C, which=which, iters=ITERS, lr=0.05, l2=1e-4)
            put(call, shape, (("W", r["W"]), ("b", r["b"]), ("loss", r["loss"])))
            r = getattr(eng, call)(nodes, labels, C, which=which, iters=2, lr=0.05, l2=1e-4, W=W, b=b)
            put(call + " from (W, b)", shape, (("W", r["W"]), ("b", r["b"]), ("loss", r["loss"])))
        pred, z = eng.classifier_predict(nodes, W, b, which=which, logits=True)
        put("classifier_predict", shape, (("pred", pred), ("logits", z)))
        put("classifier_predict no logits", shape, (("pred", eng.classifier_predict(nodes, W, b, which=which)),))
        for tag, kk in (("k", k), ("threshold", None)):
            pred, z = eng.classifier_ml_predict(nodes, W, b, which=which, k=kk, logits=True)
            put("classifier_ml_predict " + tag, shape, (("pred", pred), ("logits", z)))
            put("classifier_ml_predict %s no logits" % tag, shape, (("pred", eng.classifier_ml_predict(nodes, W, b, which=which, k=kk)),))
        for tag, kw in (("centroids", dict(centroids=cen)), ("centroid_nodes", dict(centroid_nodes=nodes[:C]))):
            r = eng.kmeans_step(nodes, which=which, **kw)
            put("kmeans_step " + tag, shape, [(n, r[n]) for n in ("assign", "dist2", "sums", "counts")] + [("inertia", np.float64(r["inertia"]))])
            r = eng.kmeans_step(nodes, which=which, sums=False, **kw)
            put("kmeans_step no sums " + tag, shape, (("assign", r["assign"]), ("dist2", r["dist2"]), ("inertia", np.float64(r["inertia"]))))
        r = eng.kmeans_fit(nodes, init=nodes[:C], max_iters=4, which=which)
        put("kmeans_fit", shape, [(n, r[n]) for n in ("centroids", "assign", "dist2", "counts", "inertia")] + [("iters", np.int32(r["iters"]))])
        for op in ("hadamard", "average", "l1", "l2"):
            r = eng.edge_classifier_lossgrad(nodes, v, ye, we, be, op=op, which=which, l2=1e-3)
            put("edge_classifier_lossgrad " + op, shape, (("loss", np.float32(r["loss"])), ("gw", r["gw"]), ("gb", np.float32(r["gb"]))))
            r = eng.edge_classifier_fit(nodes, v, ye, op=op, which=which, iters=ITERS, lr=0.05, l2=1e-4)
            put("edge_classifier_fit " + op, shape, (("w", r["w"]), ("b", np.float32(r["b"])), ("loss", r["loss"])))
            put("edge_classifier_predict " + op, shape, (("logits", eng.edge_classifier_predict(nodes, v, we, be, op=op, which=which)),))
    eng.close()

print(json.dumps({"digests": digests, "all": hashlib.sha256(json.dumps(digests, sort_keys=True).encode()).hexdigest()}))
