"""not-gpu: host logic of sample.lua's port - ganrev.sample's options, the ordering step of sortImagesByPrediction, and how
Context.l2_nearest splits more than 64 queries over calls (the library call replaced by a stub)."""
import ctypes as C

import numpy as np


def test_sample_parse_defaults_match_sample_lua():
    from ganrev import sample
    o = sample.parse([])
    assert (o.save, o.network, o.neighbours, o.colorSpace, o.writeTo) == ("logs", "adversarial.net", False, "rgb", "samples")  # sample.lua:10-14
    assert (o.seed, o.gpu, o.runs, o.noiseDim, o.noiseMethod) == (1, 0, 1, 32, "normal")                                    # :15-20
    assert (o.batchSize, o.height, o.width, o.dataset) == (16, 32, 32, "NONE")                                              # :21-24
    assert sample.image_dims(o) == (3, 32, 32) and sample.image_dims(sample.parse(["--colorSpace", "y"])) == (1, 32, 32)
    assert sample.parse(["--neighbours"]).neighbours is True


def test_prediction_order_with_ties():
    from ganrev.nn_utils import predictionOrder
    p = np.array([0.5, 0.9, 0.5, 0.1, 0.9, 0.5], np.float32)
    assert predictionOrder(p, True, 10).tolist() == [3, 0, 2, 5, 1, 4]
    assert predictionOrder(p, False, 10).tolist() == [1, 4, 0, 2, 5, 3]
    assert predictionOrder(p, False, 2).tolist() == [1, 4]
    assert predictionOrder(p.reshape(-1, 1), True, 0).tolist() == []


class _StubLib:
    """gr_l2_nearest_host / _dev: records each call's query count, answers idx = global query number, dist = k-th place"""
    def __init__(self):
        self.calls = []

    def _answer(self, qptr, q, k, idx_p, dist_p, d):
        qs = np.ctypeslib.as_array(C.cast(qptr, C.POINTER(C.c_float)), shape=(q, d))
        idx = np.ctypeslib.as_array(C.cast(idx_p, C.POINTER(C.c_int64)), shape=(q, k))
        dist = np.ctypeslib.as_array(C.cast(dist_p, C.POINTER(C.c_double)), shape=(q, k))
        idx[...] = qs[:, :1].astype(np.int64)
        dist[...] = np.arange(k)
        self.calls.append(q)
        return 0

    def gr_l2_nearest_host(self, h, table, n, d, qptr, q, k, idx_p, dist_p):
        return self._answer(qptr, q, k, idx_p, dist_p, d)


def test_l2_nearest_splits_queries_by_64():
    import ganrev._lib as L
    ctx = object.__new__(L.Context)
    ctx.lib, ctx.h = _StubLib(), None
    table = np.zeros((10, 3), np.float32)
    qs = np.repeat(np.arange(150, dtype=np.float32)[:, None], 3, axis=1)
    idx, dist = ctx.l2_nearest(table, qs, 2)
    assert ctx.lib.calls == [64, 64, 22]
    assert idx.shape == (150, 2) and (idx[:, 0] == np.arange(150)).all() and (idx[:, 1] == np.arange(150)).all()
    assert (dist == [0.0, 1.0]).all()
