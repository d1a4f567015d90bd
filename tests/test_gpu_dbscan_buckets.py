"""DBSCAN's binning by bucket population (grid.hip: k_bk_scatter, k_bk_sort). A bucket is 4096
consecutive cell ids; k_bk_sort keeps the keys and ranks of a bucket's first 6144 points in registers
and takes further rounds of the same tile for the rest. The clouds here put populations on both
sides of the old capacity (2048), of the bucket's cell count and of the new capacity into one
bucket, and mix the classes in one launch; every cloud goes through the host-planned and the
device-planned path (compact fp32 records) and through PYQSM_COORD_F32=0 (fp64 records). Labels and
core flags are the oracle's. The populations are recomputed here, so that a change of the grid
cannot quietly empty a case."""
import os

import numpy as np
import pytest

import oracle
from pyqsm_amd import hip, synth

pytestmark = pytest.mark.gpu

EPS, MIN_PTS = 0.1, 10
CAP = 6144   # grid.hip: 512 threads * kBkPer (12) points of a 4096-cell bucket in registers


def bucket_populations(P, eps=EPS):
    """Points per bucket of the grid bin_octants_* builds: cells of edge eps (1 + 2^-20) from the
    cloud's minimum, one border cell on every side, x fastest; bucket = cell id >> 12."""
    cell = eps * (1.0 + 2.0 ** -20)
    mn, mx = P.min(0), P.max(0)
    raw = (np.floor((mx - mn) / cell) + 1.0).astype(np.int64)
    dims = raw + 2
    c = np.floor((P - mn) * (1.0 / cell)).astype(np.int64)
    c = np.clip(c, 0, raw - 1) + 1
    cid = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    return np.bincount(cid >> 12, minlength=int((np.prod(dims) + 4096) >> 12)), dims


def _run(P, gpu, host=False, f64=False):
    keep = {k: os.environ.pop(k, None) for k in ("PYQSM_DBSCAN_PLAN", "PYQSM_COORD_F32")}
    if host:
        os.environ["PYQSM_DBSCAN_PLAN"] = "host"
    if f64:
        os.environ["PYQSM_COORD_F32"] = "0"
    try:
        hip.prof_enable(True, gpu)
        hip.prof_reset(gpu)
        lab, core = hip.dbscan(P, EPS, MIN_PTS, device=gpu)
        hit = hip.prof_get("dbscan_plan_hit", gpu)[1]
        miss = hip.prof_get("dbscan_plan_miss", gpu)[1]
        hip.prof_enable(False, gpu)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert hit + miss == 1
    return lab, core, "hit" if hit else "miss"


def _check_all_paths(P, gpu, representable=True):
    lab0, core0 = oracle.dbscan(P, EPS, MIN_PTS)
    # host-planned, then planned on the device with the hint the first call left; a cloud with a
    # coordinate that fp32 cannot hold is planned on the host both times (fp64 records)
    want = [("host", True, False, "miss"), ("device", False, False, "hit" if representable else "miss"),
            ("fp64 records", False, True, "miss")]
    for name, host, f64, path in want:
        lab, core, got = _run(P, gpu, host=host, f64=f64)
        assert got == path, name
        assert np.array_equal(core, core0), name
        assert np.array_equal(lab, lab0), name
    return lab0, core0


def slab(m, seed=0):
    rng = np.random.default_rng(seed)
    P = rng.uniform(0, 1, (m, 3)) * [40, 0.3, 0.1]
    return P.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("m", [63, 64, 65, 1500, 2048, 2049, 4096, 4097, CAP - 1, CAP, CAP + 1, 8192, 8193, 60_000])
def test_one_bucket_of_m_points(gpu, m):
    P = slab(m)
    pop, dims = bucket_populations(P)
    assert pop[pop > 0].tolist() == [m], "the slab is meant to fill exactly one bucket"
    _check_all_paths(P, gpu)


def test_one_bucket_is_one_cluster_at_60000(gpu):
    """The largest slab is dense enough to be one cluster of core points: ten rounds of the tile."""
    P = slab(60_000)
    lab, core, _ = _run(P, gpu)
    assert core.all() and (lab == 0).all()


def test_mixed_bucket_classes_in_one_launch(gpu):
    P = synth.forest(200_000, seed=5)
    pop, _ = bucket_populations(P)
    assert (pop == 0).any(), "empty buckets"
    assert ((pop > 0) & (pop <= 2048)).sum() > 100, "buckets of at most 2048 points"
    assert ((pop > 2048) & (pop <= CAP)).sum() >= 2, "buckets between the old and the new capacity"
    _check_all_paths(P, gpu)


def test_buckets_beyond_the_capacity_next_to_small_ones(gpu):
    """A dense slab (one bucket of several rounds) beside a sparse forest in one grid."""
    F = synth.forest(30_000, seed=3)
    S = slab(20_000, seed=1) * [0.05, 1.0, 1.0] + [F[:, 0].max() + 1.0, 0.0, 0.0]
    P = np.concatenate([F, S.astype(np.float32).astype(np.float64)])
    pop, _ = bucket_populations(P)
    assert pop.max() > CAP and ((pop > 0) & (pop <= 2048)).sum() >= 2
    _check_all_paths(P, gpu)


def test_non_representable_coordinate_takes_fp64_records(gpu):
    P = synth.forest(40_000, seed=7)
    P[123, 1] += 1e-9                      # not an fp32 value: the whole cloud keeps fp64 records
    assert np.float64(np.float32(P[123, 1])) != P[123, 1]
    pop, _ = bucket_populations(P)
    assert (pop > 0).sum() >= 2
    _check_all_paths(P, gpu, representable=False)
    S = slab(CAP + 1)
    S[5, 0] += 1e-9
    pop, _ = bucket_populations(S)
    assert pop[pop > 0].tolist() == [CAP + 1]
    _check_all_paths(S, gpu, representable=False)
