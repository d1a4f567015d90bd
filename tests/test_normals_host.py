"""Host-side checks of the normals stage: the restatement's Jacobi normals against numpy.linalg.eigh,
filter_by_norm against a literal transcription of pyQSM's get_angles + filter_by_norm, the [stem]
config section, the PointCloud normal helpers that need no GPU, and the Kruskal-with-parity
restatement on a closed sphere."""
import numpy as np
import pytest

from pyqsm_amd.geometry import point_cloud_processing as pcp
from pyqsm_amd.geometry.cloud import KDTreeSearchParamHybrid, KDTreeSearchParamKNN, PointCloud, _search_param
from pyqsm_amd.set_config import config
from tests import normals_restatement as R


def _sym(C):
    A = np.empty((len(C), 3, 3))
    A[:, 0, 0], A[:, 0, 1], A[:, 0, 2] = C[:, 0], C[:, 1], C[:, 2]
    A[:, 1, 0], A[:, 1, 1], A[:, 1, 2] = C[:, 1], C[:, 3], C[:, 4]
    A[:, 2, 0], A[:, 2, 1], A[:, 2, 2] = C[:, 2], C[:, 4], C[:, 5]
    return A


def test_jacobi_normals_match_eigh():
    rng = np.random.default_rng(0)
    X = rng.normal(size=(4000, 3, 3))
    A = X @ np.transpose(X, (0, 2, 1)) + rng.normal(size=(4000, 1, 1)) * 0.0
    C = np.stack([A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]], 1)
    n = R.jacobi_smallest(C)
    w, V = np.linalg.eigh(_sym(C))
    lam = w[:, 0]
    # residual everywhere
    r = np.linalg.norm(np.einsum("nij,nj->ni", A, n) - lam[:, None] * n, axis=1)
    assert np.all(r <= 1e-10 * np.linalg.norm(A, axis=(1, 2)))
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-14)
    # direction where the eigen-gap is clear
    gap = (w[:, 1] - w[:, 0]) > 1e-3 * w[:, 2]
    assert gap.sum() > 3000
    assert np.allclose(np.abs(np.sum(n[gap] * V[gap, :, 0], axis=1)), 1.0, atol=1e-9)


def test_restatement_normals_of_a_noisy_plane():
    rng = np.random.default_rng(1)
    P = np.c_[rng.random((3000, 2)), 1e-4 * rng.normal(size=3000)] + [5e5, 4e6, 100.0]
    N = R.estimate_normals(P, 0.1, 30)
    assert np.all(N[:, 2] > 0.99)
    table, cnt = R.neighbourhoods(P, 0.1, 30)
    C = R.covariances(P, table, cnt)
    A = _sym(C)
    lam = np.linalg.eigvalsh(A)[:, 0]
    r = np.linalg.norm(np.einsum("nij,nj->ni", A, N) - lam[:, None] * N, axis=1)
    assert np.all(r <= 1e-10 * np.linalg.norm(A, axis=(1, 2)))


def test_restatement_degenerate_and_sign():
    P = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [5, 5, 5], [5.01, 5, 5]], dtype=np.float64)
    N = R.estimate_normals(P, 0.1, 30)
    assert np.array_equal(N, np.tile([0.0, 0.0, 1.0], (6, 1)))
    prev = np.tile([0.3, 0.4, -0.5], (6, 1))
    assert np.array_equal(R.estimate_normals(P, 0.1, 30, prev), prev)


def _literal_filter(normals, t, rev=False):
    # pyQSM/math_utils/general.py:102-124 and point_cloud_processing.py:246-256, as written
    def get_angles(tup, radians=False, reference='XY'):
        if reference == 'XY':
            a = tup[0]
            b = tup[1]
            c = tup[2]
        denom = np.sqrt(a**2 + b**2)
        if denom != 0:
            radians = np.arctan(c / np.sqrt(a**2 + b**2))
            if radians:
                return radians
            else:
                return np.degrees(radians)
        else:
            return 0
    angles = np.apply_along_axis(get_angles, 1, np.asarray(normals))
    angles = np.degrees(angles)
    if rev:
        return np.where((angles < -t) | (angles > t))[0]
    return np.where((angles > -t) & (angles < t))[0]


@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("t", [10, 4, 0.5, 45])
def test_filter_by_norm_matches_the_reference(rev, t):
    rng = np.random.default_rng(2)
    N = rng.normal(size=(3000, 3))
    N /= np.linalg.norm(N, axis=1)[:, None]
    # (row 0 stays generic: apply_along_axis takes its output dtype from the first row, and an
    # integer 0 there would truncate every angle -- a quirk filter_by_norm does not copy)
    N[1:11] = [0.0, 0.0, 1.0]                  # nx = ny = 0: angle 0, kept
    N[11:21] = [0.0, 0.0, -1.0]
    N[21:31] = [0.6, 0.8, 0.0]                 # nz = 0: arctan 0
    N[31:41] = [1.0, 0.0, 0.0]
    pcd = PointCloud(rng.random((3000, 3)), normals=N)
    got = pcp.filter_by_norm(pcd, t, rev=rev)
    want = _literal_filter(N, t, rev)
    assert np.array_equal(got.points, pcd.points[want])
    assert np.array_equal(got.normals, N[want])
    assert np.array_equal(want, R.filter_by_norm_idx(N, t, rev))
    kept = set(want.tolist())
    assert all((i in kept) != rev for i in range(1, 21))  # the (0, 0, +-1) fallback normals


def test_stem_config_section_loads():
    s = config["stem"]
    assert s["normals_radius"] == 0.1 and s["normals_nn"] == 30 and s["normals_smoothing_nn"] == 50
    assert s["angle_cutoff"] == 10 and s["stem_voxel_size"] == "" and s["post_id_stat_down"] is False
    assert s["stem_neighbors"] == 10 and s["stem_ratio"] == 2 and s["stem_iters"] == 3
    from pyqsm_amd import qsm_generation
    d = dict(zip(qsm_generation.get_stem_pcd.__code__.co_varnames[2:9], qsm_generation.get_stem_pcd.__defaults__[2:9]))
    assert d == {"normals_radius": 0.1, "normals_nn": 30, "nb_neighbors": 10, "std_ratio": 2,
                 "angle_cutoff": 10, "voxel_size": "", "post_id_stat_down": False}


def test_search_params_and_normal_helpers():
    assert _search_param(KDTreeSearchParamHybrid(radius=0.1, max_nn=30)) == (0.1, 30)
    assert _search_param(KDTreeSearchParamKNN(12)) == (None, 12)
    assert _search_param(None) == (None, 30)
    P = np.arange(12.0).reshape(4, 3)
    pcd = PointCloud(P, normals=[[3.0, 4.0, 0.0], [0, 0, 0], [0, 0, 2.0], [1, 1, 1]])
    assert pcd.has_normals() and not PointCloud(P).has_normals()
    pcd.normalize_normals()
    assert np.array_equal(pcd.normals[:3], [[0.6, 0.8, 0.0], [0, 0, 0], [0, 0, 1.0]])
    sub = pcd.select_by_index([2, 0])
    assert np.array_equal(sub.normals, pcd.normals[[2, 0]])
    inv = pcd.select_by_index([1], invert=True)
    assert np.array_equal(inv.normals, pcd.normals[[0, 2, 3]])
    with pytest.raises(ValueError):
        pcd.orient_normals_consistent_tangent_plane(10, 0.5)
    with pytest.raises(ValueError):
        pcd.orient_normals_consistent_tangent_plane(10, cos_alpha_tol=0.9)
    with pytest.raises(RuntimeError):
        PointCloud(P).orient_normals_consistent_tangent_plane(10)


def _sphere(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def test_kruskal_orients_a_sphere_outward():
    S = _sphere(4000, 3)
    P = 2.0 * S + [1.0, -2.0, 3.0]
    rng = np.random.default_rng(4)
    N = np.where(rng.random(4000)[:, None] < 0.5, -S, S)   # true normals, random signs
    O = R.orient_tangent_plane(P, N, 12)
    assert np.all(np.sum(O * S, axis=1) > 0)


def test_kruskal_roots_each_component_at_its_highest_point():
    S = _sphere(800, 5)
    P = np.r_[S, S + [100.0, 0, 0]]
    N = np.r_[-S, S]
    O = R.orient_tangent_plane(P, N, 10)
    assert np.all(np.sum(O * np.r_[S, S], axis=1) > 0)
