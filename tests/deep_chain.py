"""Points on a line whose kNN graph hooks into ONE tree of depth m - 2 in the first Boruvka round
(csrc/boruvka.hpp): every point but the last has the edge to its successor as its lightest incident
edge, so round 1 hooks 0 -> 1 -> ... -> m-2 <- m-1. What the bounded pointer jumping and the parity
composition have to get right. The tests of the skeleton forest and of the normal orientation build
their weights on it and state the precondition here, in NumPy, before they call the GPU."""
import numpy as np


def relabel(m, permuted, seed):
    """label[i]: the index that the i-th point along the line gets in the cloud."""
    return np.random.default_rng(seed).permutation(m) if permuted else np.arange(m)


def line_graph(t, k):
    """The undirected kNN graph (k others per point) of points at the ascending positions t, as
    pairs a < b of positions. No tie at the cut, so the graph does not depend on the labels."""
    m = len(t)
    j = np.arange(m)[:, None] + np.r_[-np.arange(1, k + 1), np.arange(1, k + 1)]
    inside = (j >= 0) & (j < m)
    d = np.where(inside, np.abs(t[np.clip(j, 0, m - 1)] - t[:, None]), np.inf)
    o = np.argsort(d, axis=1, kind="stable")
    ds = np.take_along_axis(d, o, axis=1)
    assert (ds[:, k - 1] < ds[:, k]).all()
    nb = np.take_along_axis(j, o, axis=1)[:, :k].ravel()
    i = np.repeat(np.arange(m), k)
    pairs = np.unique(np.stack([np.minimum(i, nb), np.maximum(i, nb)], axis=1), axis=0)
    return pairs[:, 0], pairs[:, 1]


def assert_one_chain(a, b, w, label):
    """The precondition: the weights w of the edges {a, b} are strictly ordered, and under (weight,
    smaller label, larger label) the lightest edge at position i < m - 1 is {i, i + 1}."""
    m = len(label)
    assert len(np.unique(w)) == len(w)
    end, other, ww = np.r_[a, b], np.r_[b, a], np.r_[w, w]
    lo, hi = np.minimum(label[end], label[other]), np.maximum(label[end], label[other])
    o = np.lexsort((hi, lo, ww, end))
    first = np.r_[True, end[o][1:] != end[o][:-1]]
    assert np.array_equal(end[o][first], np.arange(m))
    assert np.array_equal(other[o][first][:m - 1], np.arange(1, m))
