"""What the device tests of the node-classification path share (test_gpu_node_classification.py and its multi-label twin): two
random tables and one engine per embedding width, made once, and the comparison against the (float64, float32) restatements
under the derived tolerance classifier_ref.tol."""
import numpy as np

from tests.support.classifier_ref import tol

N_TABLE = 5000
_tables = {}
_engines = {}


def tables(d):
    """two different tables [N_TABLE, d] (generator, discriminator), made once per d"""
    if d not in _tables:
        rs = np.random.RandomState(100 + d)
        _tables[d] = ((0.3 * rs.randn(N_TABLE, d)).astype(np.float32), (0.3 * rs.randn(N_TABLE, d) + 0.05).astype(np.float32))
    return _tables[d]


def engine_of(d):
    """the engine on ``tables(d)``, made once per d (until ``close_engines``)"""
    if d not in _engines:
        import graphgan_amd
        _engines[d] = graphgan_amd.Engine(*tables(d))
    return _engines[d]


def close_engines():
    for e in _engines.values():
        e.close()
    _engines.clear()


def compare(tag, names, got, r64, r32):
    """every ``got`` within tol(float32 reference, float64 reference) of the float64 reference"""
    for name, g, w64, w32 in zip(names, got, r64, r32):
        t = tol(w32, w64)
        err = float(np.max(np.abs(np.asarray(g, dtype=np.float64) - w64)))
        print("%s %s: err %.3g tol %.3g" % (tag, name, err, t))
        assert err <= t, (tag, name, err, t)
