"""tests/epiphyte_restatement.py held to NumPy, to scikit-learn's recorded results
(tests/golden/kmeans_sklearn.npz, written by tests/golden/make_kmeans_golden.py) and to the
reference's formulation of the percentile splits. No GPU."""
import functools
import os

import numpy as np
import pytest

from pyqsm_amd.geometry import stem_width as sw
from pyqsm_amd.math_utils.clustering import kmeanspp_draws
from tests import epiphyte_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmeans_sklearn.npz")

# The restatement against scikit-learn 1.7.2 when the goldens were written: centres within 7.2e-15
# (coordinates of order 10), inertia within 3.3e-16 relative. The bounds are 100 times that, far below
# the 1e-10 the silhouette tests use.
CENTRE_BOUND = 7.2e-13
INERTIA_REL_BOUND = 3.3e-14


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def golden_case(name):
    g = golden()
    k, seed = (int(v) for v in g[f"{name}_k_seed"])
    return g[f"{name}_x"].astype(np.float64), k, seed, g


GOLDEN_NAMES = ["tree", "box", "blobs", "plane", "feature"]


def test_golden_names():
    assert list(golden()["names"]) == GOLDEN_NAMES
    assert os.path.getsize(GOLDEN) < 200_000


@pytest.mark.parametrize("name", GOLDEN_NAMES)
@pytest.mark.parametrize("fn", [R.kmeans_pp, R.kmeans_pp_plain], ids=["chunk", "plain"])
def test_restatement_reproduces_sklearn(name, fn):
    x, k, seed, g = golden_case(name)
    first, u = kmeanspp_draws(len(x), k, seed)
    r = fn(x, k, first, u)
    assert np.array_equal(r.seeds, g[f"{name}_seeds"])
    assert np.array_equal(r.labels, g[f"{name}_labels"])
    assert r.n_iter == int(g[f"{name}_n_iter"])
    dc = np.abs(r.centres - g[f"{name}_centres"]).max()
    di = abs(r.inertia - float(g[f"{name}_inertia"])) / float(g[f"{name}_inertia"])
    print(f"{name}: centres {dc:.3e}, inertia (relative) {di:.3e}")
    if fn is R.kmeans_pp:
        assert dc <= CENTRE_BOUND < 1e-10
        assert di <= INERTIA_REL_BOUND < 1e-10


@pytest.mark.parametrize("n,k,seed", [(1, 1, 0), (20, 20, 3), (3000, 20, 0), (2000, 2, 7), (513, 64, 11)])
def test_draws_equal_a_randomstate_replay(n, k, seed):
    first, u = kmeanspp_draws(n, k, seed)
    rs = np.random.RandomState(seed)
    T = 2 + int(np.log(k))
    assert first == rs.choice(n, p=np.full(n, 1.0) / float(n))
    assert u.shape == ((k - 1) * T,)
    for c in range(k - 1):
        assert np.array_equal(u[c * T:(c + 1) * T], rs.uniform(size=T))
    assert ((u >= 0) & (u < 1)).all()


def test_draws_are_what_sklearn_draws():
    """The recorded k-means++ indices start with the drawn first index."""
    for name in GOLDEN_NAMES:
        x, k, seed, g = golden_case(name)
        assert kmeanspp_draws(len(x), k, seed)[0] == int(g[f"{name}_seeds"][0])


@pytest.mark.parametrize("n", [1, 2, 257])
@pytest.mark.parametrize("q", [0, 60, 65, 100])
def test_percentile_equals_numpy(n, q):
    rng = np.random.default_rng(10 * n + q)
    for v in (rng.normal(0, 1, n), rng.normal(0, 1e-310, n), np.round(rng.normal(0, 2, n)), np.full(n, -3.25)):
        want = np.percentile(v, q)
        got = R.percentile(v, q)
        assert got.tobytes() == np.float64(want).tobytes() or (got == 0 and want == 0)
        lo, hi, t = sw.percentile_ranks(n, q)          # the helper the wrappers share with the stem width
        s = np.sort(v)
        assert float(sw.lerp(s[lo], s[hi], t)) == want
        assert R.percentile_ranks(n, q) == (int(lo), int(hi), float(t))


def test_select_orders_negative_keys_and_zeros():
    v = np.array([3.0, -0.0, 0.0, -2.5, 5e-324, -5e-324, -np.inf, np.inf, 1.0])
    got = R.select(v, np.arange(len(v)))
    assert np.array_equal(got, np.sort(v))
    assert not np.signbit(got[got == 0]).any()
    with pytest.raises(ValueError):
        R.select(np.array([1.0, np.nan]), [0])


def test_partition_equals_the_reference_formulation():
    """identify_epiphytes: c_mag by np.linalg.norm per row, np.where(v > np.percentile(v, q))."""
    shift = R.shift_field(20_000, seed=4)
    labels, thr, counts = R.shift_components(shift, 65, 60)
    c_mag = np.array([np.linalg.norm(x) for x in shift])
    high = np.where(c_mag > np.percentile(c_mag, 65))[0]
    z_mag = np.array([x[2] for x in shift[high]])
    leaves = high[np.where(z_mag > np.percentile(z_mag, 60))[0]]
    epis = np.setdiff1d(high, leaves)
    assert np.array_equal(np.nonzero(labels > 0)[0], high)
    assert np.array_equal(np.nonzero(labels == 1)[0], leaves)
    assert np.array_equal(np.nonzero(labels == 2)[0], epis)
    assert counts.tolist() == [len(shift) - len(high), len(leaves), len(epis)]
    assert thr[1] == np.percentile(z_mag, 60)


def test_shift_components_degenerate():
    labels, thr, counts = R.shift_components(np.zeros((0, 3)))
    assert len(labels) == 0 and np.isnan(thr).all() and counts.tolist() == [0, 0, 0]
    labels, thr, counts = R.shift_components(np.ones((7, 3)))          # nothing above the percentile
    assert counts.tolist() == [7, 0, 0] and np.isnan(thr[1])


def test_restatement_edge_rules():
    # zero potential: five distinct positions, eight centres -> index 0 is drawn again, empty centres stay
    x = R.cloud("few", 300, seed=3)
    first, u = kmeanspp_draws(300, 8, 0)
    r = R.kmeans_pp(x, 8, first, u)
    assert r.n_empty >= 3 and 0 in r.seeds[5:]
    assert r.inertia <= 1e-25
    # chunk sum against math.fsum
    import math
    v = np.random.default_rng(0).normal(0, 1, 1000)
    assert abs(R.chunk_sum(v) - math.fsum(v)) < 1e-12
    # the sampling scan: a running sum that reaches r exactly at a point selects that point
    c = np.ones(600)
    assert R.sample(c, 256.0) == 255 and R.sample(c, 256.5) == 256 and R.sample(c, 0.0) == 0
    assert R.sample(c, 600.0) == 599 and R.sample(c, 1e9) == 599
