"""laplacian.hip against oracle.point_cloud_laplacian on the inputs of tests/laplacian_cases.py: the fan
kernel of k > 32 and the dead half-wave of an odd n, edge buckets at and beyond k_glue_wave's 64 records,
rows on both sides of every limit of k_sort_rows, rows of up to 26 chunks in k_rows_wave with the diagonal
first, mid-row and last, neighbour lists with empty places (n <= k), the two switches and the segmented
call. tests/test_laplacian_cases_host.py proves on the CPU that each input has the sizes its table entry
names; here the trace (PYQSM_LBC_TRACE) says that the device saw the same sizes, so a moved threshold
fails the test instead of silently moving a case to another path.

Bounds are those of tests/test_gpu_laplacian.py: the pattern equal, values within 1e-9 of the largest
entry, mass within 1e-9 of the largest mass, L - L.T exactly zero, a second call the same bytes."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from scipy.sparse import block_diag, csr_matrix

from pyqsm_amd import hip

from tests import laplacian_cases as lc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = re.compile(r"laplacian rows: (\d+) contributions at most, (\d+) rows beyond the wave path\n")
BUCKETS = re.compile(r"laplacian edge buckets: (\d+) records at most, (\d+) buckets beyond the wave path\n")
LINE = re.compile(r"^(\S+): equal to the oracle, data (\S+) mass (\S+) sha256 ([0-9a-f]{64})$", re.M)

OFF = re.compile(r"^    off-diagonal values sha256 ([0-9a-f]{64})$", re.M)

_default = {}


def _same_bytes(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes()
               for x, y in zip((*a[0], a[1]), (*b[0], b[1])))


def _build(case, gpu):
    (indptr, indices, data), mass = hip.pc_laplacian(case.points, case.k, lc.MOLL, device=gpu)
    return (indptr.copy(), indices.copy(), data.copy()), mass.copy()


def default_result(case, gpu):
    """The default path's result of a case, built once per process (every test asks for it before it sets
    a switch)."""
    if case.name not in _default:
        _default[case.name] = _build(case, gpu)
    return _default[case.name]


@pytest.mark.parametrize("case", lc.CASES, ids=repr)
def test_case_matches_oracle_on_the_path_it_names(gpu, case, monkeypatch, capfd):
    first = default_result(case, gpu)
    monkeypatch.setenv("PYQSM_LBC_TRACE", "1")
    capfd.readouterr()
    got = _build(case, gpu)
    err = capfd.readouterr().err
    monkeypatch.delenv("PYQSM_LBC_TRACE")
    bad, d_data, d_mass = lc.differences(got, lc.expected(case))
    print(f"{case.name}: {case.fans_class}, {case.bucket_class} (bucket {case.bucket}), {case.row_class} "
          f"(row {case.row}): data differs by {d_data:.1e} of the largest entry, mass by {d_mass:.1e}")
    assert not bad, "; ".join(bad)
    assert _same_bytes(first, got)                               # a second call: the same bytes
    # the device saw the sizes the oracle counted: the paths the table names are the paths that ran
    bucket, rows = lc.counts(case)
    seen_rows, seen_buckets = ROWS.findall(err), BUCKETS.findall(err)
    assert seen_rows == [(str(rows.max()), str((rows > 64 * 8).sum()))], err[-2000:]
    assert seen_buckets == [(str(bucket.max()), str((bucket > 64).sum()))], err[-2000:]
    assert rows.max() == case.row and bucket.max() == case.bucket


@pytest.mark.parametrize("name", lc.PUSH_ALL_CASES)
def test_push_all_makes_the_same_flips(gpu, name, monkeypatch):
    """PYQSM_FLIP_PUSH_ALL=1 (read per call): a flip lists its four outer edges unseen. Longer lists, the
    same flips, the same bytes."""
    case = lc.BY_NAME[name]
    want = default_result(case, gpu)
    monkeypatch.setenv("PYQSM_FLIP_PUSH_ALL", "1")
    got = _build(case, gpu)
    assert _same_bytes(want, got)
    assert not lc.differences(got, lc.expected(case))[0]


@pytest.fixture(scope="module")
def thread_per_row_child(gpu):
    """PYQSM_LAP_ROWS=0 (k_rows, a thread per row) is read once per process: ONE fresh child runs the
    whole table against the oracle (laplacian_cases.main) and prints a digest of every case's values."""
    env = dict(os.environ, PYQSM_LAP_ROWS="0")
    env.pop("PYQSM_FLIP_PUSH_ALL", None)
    env.pop("PYQSM_LBC_TRACE", None)
    code = ("import sys; sys.path.insert(0, sys.argv[1]); from tests import laplacian_cases as lc; "
            "sys.exit(lc.main())")
    return subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, env=env, cwd=ROOT,
                          timeout=120)


def test_thread_per_row_kernel_matches_the_oracle(gpu, thread_per_row_child):
    """k_rows on every case of the table: the oracle's pattern, values and mass within the bounds above,
    L symmetric to the bit. And its OFF-DIAGONAL values are the default path's to the bit, on every
    case: both kernels add a column's contributions one after the other in the sorted (column, key)
    order, which is what the comment in k_rows_wave claims."""
    r = thread_per_row_child
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert [m[1] for m in LINE.finditer(r.stdout)] == [c.name for c in lc.CASES]
    off = OFF.findall(r.stdout)
    assert len(off) == len(lc.CASES)
    for case, got in zip(lc.CASES, off):
        assert got == lc.digest(lc.off_diagonal(default_result(case, gpu)[0])), case.name


def test_thread_per_row_kernel_gives_the_default_paths_bytes_on_the_longest_rows(gpu, thread_per_row_child):
    """On the three longest rows (the hubs of 180) k_rows' values are byte-equal to k_rows_wave's,
    diagonal included - and so they are on every other case of the table.

    This test found that they were not: k_rows_wave used to subtract, per chunk of 64 contributions, a
    butterfly sum over the lanes from the diagonal, where k_rows (and the oracle) subtract the merged
    columns one after the other. The off-diagonal bytes were equal, the diagonals 1 to 3 ulp apart (at most
    2.3e-16 of the largest entry) in 2, 29 and 56 of the 181 rows of the three hubs of 180 and in about a
    third of the rows of the forests. k_rows_wave now subtracts column by column as well."""
    r = thread_per_row_child
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = {m[1]: m[4] for m in LINE.finditer(r.stdout)}
    for name in lc.LONGEST_ROWS:
        want = lc.digest(default_result(lc.BY_NAME[name], gpu)[0][2])
        print(f"{name}: k_rows {lines[name]}, k_rows_wave {want}")
    for name in lc.LONGEST_ROWS:
        assert lines[name] == lc.digest(default_result(lc.BY_NAME[name], gpu)[0][2]), name
    for case in lc.CASES:
        assert lines[case.name] == lc.digest(default_result(case, gpu)[0][2]), case.name


def test_segmented_call_is_the_block_diagonal_of_the_oracles(gpu):
    """pyqsm_pc_laplacian_seg on [hub(70), forest(801), two-centre hub] at k = 32: every block is the
    oracle's Laplacian of that cloud alone, built with the cloud's OWN mollification length (k_seg_eps,
    k_tri_eps) - at a mollify factor of 1e-3 the forest's is positive and the hubs' are zero, so one
    shared length would change the hubs' blocks (the host test shows that on the oracle)."""
    segs = lc.segments()
    P = np.concatenate(segs)
    start = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    got = hip.pc_laplacian(P, lc.SEG_K, lc.SEG_MOLL, device=gpu, seg_start=start)
    parts = [lc.expected_segment(j) for j in range(len(segs))]
    want = block_diag([q[0] for q in parts], format="csr")
    want.sort_indices()
    want = csr_matrix((want.data, want.indices.astype(np.int32), want.indptr.astype(np.int32)), shape=want.shape)
    mass = np.concatenate([q[1] for q in parts])
    bad, d_data, d_mass = lc.differences(got, (want, mass))
    print(f"segmented call: data differs by {d_data:.1e} of the largest entry, mass by {d_mass:.1e}")
    assert not bad, "; ".join(bad)
    again = hip.pc_laplacian(P, lc.SEG_K, lc.SEG_MOLL, device=gpu, seg_start=start)
    assert _same_bytes(got, again)
    # and per block, with each block's own scale (the forest's entries are the largest of the stack)
    (indptr, indices, data), m = got
    L = csr_matrix((data, indices, indptr), shape=want.shape)
    for j, (L0, M0) in enumerate(parts):
        b, e = start[j], start[j + 1]
        blk = L[b:e, b:e].tocsr()
        blk.sort_indices()
        assert blk.nnz == L0.nnz and np.array_equal(blk.indices, L0.indices)
        assert np.abs(blk.data - L0.data).max() <= 1e-9 * np.abs(L0.data).max(), j
        assert np.abs(m[b:e] - M0).max() <= 1e-9 * M0.max(), j
