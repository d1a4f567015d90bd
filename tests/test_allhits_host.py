"""The MIRROR oracle of the all-hits path (oracle.list_intersections: the fp32 operation sequence of
k_all_hits in raycast.hip) against the independent fp64 evaluation of oracle/ray_f64.c over ALL
ray x triangle pairs, on the three cases of tests/allhits_cases.py. No GPU: the GPU tests hold the
kernels bit-equal to this mirror, so what is wrong here is wrong there. It also keeps the comparison
itself honest: a dropped record, an invented record and two swapped records must each be reported.

Measured on the CPU (fp64 hits / disagreements, all explained / worst relative t over all hits):
sun 1019 / 0 / 1.0e-6, sun_low 1382 / 1 / 1.1e-6, general 1822 / 0 / 6.1e-6; every case prints
its record."""
import numpy as np
import pytest

import oracle

from tests import allhits_cases as ac


@pytest.mark.parametrize("name", list(ac.CASES))
def test_mirror_all_hits_against_fp64(name):
    v, t, rays = ac.case(name)
    assert len(rays) == ac.N_RAYS
    rec = ac.compare_all_hits(oracle.list_intersections(v, t, rays), v, t, rays)
    print(f"{name} (mirror) vs fp64:", rec)
    ac.check_record(rec)
    assert rec["pairs"] == len(rays) * len(t) and rec["fp64_hits"] > 1000


def test_fp64_all_pairs_on_known_answers():
    """One triangle in z = 0: through the interior from both sides, behind the origin, outside,
    parallel to the plane."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    t = np.array([[0, 1, 2], [0, 0, 0]], np.int32)                    # and a zero-area triangle
    rays = np.array([[0.25, 0.5, 2, 0, 0, -1], [0.25, 0.5, -3, 0, 0, 2], [0.25, 0.5, 2, 0, 0, 1],
                     [0.75, 0.75, 2, 0, 0, -1], [0.25, 0.5, 2, 1, 0, 0]], np.float32)
    hit, tt, bary = ac.fp64_all_pairs(v, t, rays)
    assert hit.shape == (5, 2) and tt.shape == (5, 2) and bary.shape == (5, 2, 3)
    assert hit[:, 0].tolist() == [True, True, False, False, False] and not hit[:, 1].any()
    assert tt[:3, 0].tolist() == [2.0, 1.5, -2.0]
    assert np.array_equal(bary[0, 0], [0.25, 0.25, 0.5])             # weights of v0, v1, v2
    assert np.isnan(tt[4, 0]) and np.isnan(tt[:, 1]).all()
    assert ac.fp64_all_pairs(v, t[:0], rays)[0].shape == (5, 0)


@pytest.fixture(scope="module")
def sun():
    v, t, rays = ac.case("sun")
    ref = oracle.list_intersections(v, t, rays)
    for a in ref.values():
        a.setflags(write=False)
    return v, t, rays, ref


def _without(ref, k):
    out = {key: np.delete(ref[key], k, axis=0) for key in ac.KEYS if key != "counts"}
    out["counts"] = np.array(ref["counts"])
    out["counts"][ref["ray_ids"][k]] -= 1
    return out


def _with(ref, k, ray, prim, t, uv):
    out = {"ray_ids": np.insert(ref["ray_ids"], k, ray), "primitive_ids": np.insert(ref["primitive_ids"], k, prim),
           "t_hit": np.insert(ref["t_hit"], k, t), "primitive_uvs": np.insert(ref["primitive_uvs"], k, uv, axis=0),
           "counts": np.array(ref["counts"])}
    out["counts"][ray] += 1
    return out


def test_a_dropped_record_is_reported(sun):
    """One real crossing, well inside its triangle, removed (counts kept consistent): the structure
    holds, fp64 reports the missing crossing as an unexplained disagreement."""
    v, t, rays, ref = sun
    _, _, b64 = ac.fp64_all_pairs(v, t, rays)
    inner = b64[ref["ray_ids"].astype(np.int64), ref["primitive_ids"].astype(np.int64)].min(1) > 0.05
    k = int(np.flatnonzero(inner)[len(np.flatnonzero(inner)) // 2])
    base = ac.compare_all_hits(ref, v, t, rays)
    rec = ac.compare_all_hits(_without(ref, k), v, t, rays)
    assert rec["structure"] == []
    assert rec["disagreements"] == base["disagreements"] + 1 and rec["unexplained"] == 1
    assert rec["unexplained_pairs"] == [(int(ref["ray_ids"][k]), int(ref["primitive_ids"][k]))]
    with pytest.raises(AssertionError):
        ac.check_record(rec)


def test_an_invented_record_is_reported(sun):
    """One record added, in order, for a pair whose line misses the triangle by a wide margin."""
    v, t, rays, ref = sun
    _, _, b64 = ac.fp64_all_pairs(v, t, rays)
    ray, prim = map(int, np.argwhere(b64.min(2) < -0.5)[len(rays) * len(t) // 4])
    key = ref["ray_ids"].astype(np.int64) * len(t) + ref["primitive_ids"]
    k = int(np.searchsorted(key, ray * len(t) + prim))
    rec = ac.compare_all_hits(_with(ref, k, ray, prim, 1.0, (0.3, 0.3)), v, t, rays)
    assert rec["structure"] == []
    assert rec["unexplained"] == 1 and rec["unexplained_pairs"] == [(ray, prim)]
    with pytest.raises(AssertionError):
        ac.check_record(rec)


def test_swapped_records_are_reported(sun):
    """Two adjacent records of one ray exchanged: the same set of pairs, so fp64 has nothing to say;
    the order check does."""
    v, t, rays, ref = sun
    ray = int(np.flatnonzero(ref["counts"] >= 2)[0])
    k = int(ac.split_by_ray(ref)[0][ray])
    out = ac.copy_result(ref)
    for key in ac.KEYS[1:]:
        out[key][[k, k + 1]] = out[key][[k + 1, k]]
    rec = ac.compare_all_hits(out, v, t, rays)
    assert rec["unexplained"] == 0 and rec["disagreements"] == ac.compare_all_hits(ref, v, t, rays)["disagreements"]
    assert len(rec["structure"]) == 1 and "ascending" in rec["structure"][0]
    with pytest.raises(AssertionError):
        ac.check_record(rec)


def test_wrong_counts_and_duplicates_are_reported(sun):
    v, t, rays, ref = sun
    out = ac.copy_result(ref)
    out["counts"][[0, 1]] = out["counts"][[1, 0]] + np.int32([1, -1])    # same sum, another histogram
    assert any("histogram" in s for s in ac.compare_all_hits(out, v, t, rays)["structure"])
    k = len(ref["ray_ids"]) // 2
    dup = _with(ref, k, int(ref["ray_ids"][k]), int(ref["primitive_ids"][k]), ref["t_hit"][k],
                ref["primitive_uvs"][k])
    assert any("duplicate" in s for s in ac.compare_all_hits(dup, v, t, rays)["structure"])
    far = ac.copy_result(ref)
    far["primitive_ids"][-1] = len(t)                                    # an id past the mesh: reported, not indexed
    assert any("out of range" in s for s in ac.compare_all_hits(far, v, t, rays)["structure"])
    short = ac.copy_result(ref)
    short["counts"][int(ref["ray_ids"][0])] += 1
    assert any("sum" in s for s in ac.compare_all_hits(short, v, t, rays)["structure"])
