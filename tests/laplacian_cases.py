"""Inputs shared by tests/test_laplacian_cases_host.py (the CPU proof, from the oracle's counts alone,
that every input reaches the kernel class its table entry names) and tests/test_gpu_laplacian_classes.py
(laplacian.hip against oracle.point_cloud_laplacian on those inputs).

laplacian.hip picks its path by three sizes: the neighbour count (k_fans<2>, a half-wave per point, up to
k = 32; k_fans<1> beyond), the length of a vertex's edge bucket (k_glue_wave up to 64 records, k_glue
beyond) and the number of contributions in a row (sort_row_wave<1, 2, 4, 8> up to 64, 128, 256 and 512,
one lane's insertion sort beyond; k_rows_wave walks the row in chunks of 64). The forest clouds of the
rest of the suite stay below 150 contributions a row. What grows a row and a bucket while the cloud stays
at a few dozen points is a HUB:

  hub(M, seed, centre_row)       one centre inside a convex ring of M points. Every ring point's fan holds
                                 the centre, and after the flips the centre still has all M ring points as
                                 neighbours: its row and (as the smaller endpoint of every spoke) its edge
                                 bucket grow linearly with M.
  two_centre_hub(M, seed, gap)   a second centre `gap` beside the first: two long rows of nearly the same
                                 length, which land on both sides of a limit.
  hub_beside_forest(forest_first) forest(800) and a hub of 70 moved by (10, 0, 0), in both orders: the long
                                 row and the long bucket in a cloud of several blocks.
  sheet(n, seed)                 n points of a thin random sheet, for n <= k.

Every cloud is in general position (no four ring points co-circular, no ties among the neighbours): the
pattern of L does not change under coordinate noise of 1e-13 (the host test holds that), so kernel and
oracle, which differ by rounding a thousand times smaller, must agree on it.

Every case is built once per process from fixed seeds and is read-only; expected() and counts() keep
the oracle's answers, so that tests which share an input share them."""
import functools
import hashlib

import numpy as np

import oracle
from pyqsm_amd import synth

MOLL = 1e-6
SHIFT = np.array([3.0, -2.0, 1.0])
CENTRE = np.array([0.07, -0.03, 0.0])
BUCKET_WAVE_MAX = 64                 # k_glue_wave takes buckets up to this many records
ROW_LIMITS = (64, 128, 256, 512)     # sort_row_wave<1>, <2>, <4>, <8>; the serial sort beyond


def frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _ring(M, seed):
    rng = np.random.default_rng(seed)
    a = (np.arange(M) + rng.uniform(-0.3, 0.3, M)) * (2.0 * np.pi / M)
    z = rng.normal(0.0, 0.002, M)
    r = 1.0 + 0.15 * np.cos(a)          # convex, and no four points on one circle
    return np.stack([r * np.cos(a), r * np.sin(a), z], 1)


@functools.lru_cache(maxsize=None)
def hub(M, seed=0, centre_row=0):
    """M ring points and the centre, which sits at row `centre_row` (0 .. M)."""
    ring = _ring(M, seed)
    return frozen(np.concatenate([ring[:centre_row], CENTRE[None], ring[centre_row:]]) + SHIFT)


@functools.lru_cache(maxsize=None)
def two_centre_hub(M, seed=0, gap=0.01):
    """The ring with two centres `gap` apart in x, at rows 0 and 1."""
    return frozen(np.concatenate([CENTRE[None], CENTRE[None] + [gap, 0.0, 0.0], _ring(M, seed)]) + SHIFT)


@functools.lru_cache(maxsize=None)
def forest(n, seed):
    return frozen(synth.forest(n, seed))


N_FOREST_BESIDE, M_HUB_BESIDE = 800, 70


@functools.lru_cache(maxsize=None)
def hub_beside_forest(forest_first):
    parts = [forest(N_FOREST_BESIDE, N_FOREST_BESIDE), hub(M_HUB_BESIDE) + [10.0, 0.0, 0.0]]
    return frozen(np.concatenate(parts if forest_first else parts[::-1]))


@functools.lru_cache(maxsize=None)
def sheet(n, seed):
    rng = np.random.default_rng(seed)
    return frozen(rng.normal(0.0, 1.0, (n, 3)) * [1.0, 1.0, 0.05] + SHIFT)


_CLOUDS = {"hub": hub, "two_centre_hub": two_centre_hub, "forest": forest,
           "hub_beside_forest": hub_beside_forest, "sheet": sheet}


def row_class(m):
    """The sorting path of a row of m contributions (k_sort_rows)."""
    for per, limit in zip((1, 2, 4, 8), ROW_LIMITS):
        if m <= limit:
            return f"sort_row_wave<{per}>"
    return "serial sort"


def bucket_class(m):
    return "k_glue_wave" if m <= BUCKET_WAVE_MAX else "k_glue"


def fans_class(n, k):
    if k > 32:
        return "k_fans<1>"
    return "k_fans<2>, dead half-wave" if n % 2 else "k_fans<2>"


class Case:
    """One input of the table: cloud(*args) at k neighbours; `row` and `bucket` are the longest row and
    the longest edge bucket that the oracle counted for it (mollify factor MOLL), and the three class
    names say which paths of laplacian.hip they select."""

    def __init__(self, name, cloud, args, k, row, bucket):
        self.name, self.cloud, self.args, self.k, self.row, self.bucket = name, cloud, args, k, row, bucket
        self.row_class, self.bucket_class = row_class(row), bucket_class(bucket)

    @property
    def points(self):
        return _CLOUDS[self.cloud](*self.args)

    @property
    def fans_class(self):
        return fans_class(len(self.points), self.k)

    def __repr__(self):
        return self.name


def _hub(M, k, row, bucket, seed=0, centre_row=0):
    return Case(f"hub{M}_s{seed}_c{centre_row}_k{k}", "hub", (M, seed, centre_row), k, row, bucket)


# Lengths measured with oracle.point_cloud_laplacian_counts; tests/test_laplacian_cases_host.py holds the
# oracle to every one of them. A row of a hub has an even number of contributions, and below ~170 a
# multiple of four: 128 and 132 are the nearest pair around that limit that M, k and the seeds 0..49 give
# (256 | 258 and 512 | 514 exist).
CASES = (
    # the limits of k_sort_rows, both sides, and one hub per class between them
    _hub(6, 3, row=64, bucket=28, seed=10),            # sort_row_wave<1>, full
    _hub(4, 3, row=68, bucket=20, seed=2),             # <2>, the next length found above 64
    _hub(8, 6, row=92, bucket=44),
    _hub(11, 9, row=128, bucket=62, seed=1),           # <2>, full
    _hub(11, 11, row=132, bucket=66),                  # <4>; bucket: the next size above 64
    _hub(12, 8, row=132, bucket=64),                   # bucket exactly at k_glue_wave's limit
    _hub(13, 8, row=132, bucket=66),
    _hub(16, 12, row=180, bucket=88),
    _hub(24, 12, row=234, bucket=118),
    _hub(27, 12, row=256, bucket=130),                 # <4>, full
    _hub(27, 12, row=258, bucket=130, seed=2),         # <8>
    _hub(40, 20, row=388, bucket=198),
    _hub(40, 20, row=388, bucket=105, centre_row=20),
    _hub(40, 20, row=388, bucket=9, centre_row=40),    # the centre is the larger end of every spoke
    _hub(55, 20, row=506, bucket=258),
    _hub(56, 20, row=512, bucket=262, seed=1),         # <8>, full
    _hub(56, 20, row=514, bucket=262, seed=2),         # serial sort
    _hub(70, 32, row=662, bucket=342),                 # k = 32 fills the half-wave
    _hub(180, 64, row=1602, bucket=846),               # k_fans<1>; 26 chunks of 64 in k_rows_wave
    _hub(180, 64, row=1606, bucket=443, centre_row=90),   # diagonal slotted in mid-row
    _hub(180, 64, row=1602, bucket=9, centre_row=180),    # ... and at the row's end
    # two long rows in one cloud
    Case("two_centres40_gap0.01_k20", "two_centre_hub", (40, 0, 0.01), 20, row=252, bucket=124),
    Case("two_centres40_gap0.05_k32", "two_centre_hub", (40, 0, 0.05), 32, row=258, bucket=132),  # 258 | 234
    # the long row and bucket among ordinary ones, first and last in the cloud
    Case("forest800_then_hub70_k32", "hub_beside_forest", (True,), 32, row=662, bucket=342),
    Case("hub70_then_forest800_k32", "hub_beside_forest", (False,), 32, row=662, bucket=342),
    # every k around the two fan kernels' limit, n odd: the last wave of k_fans<2> has a dead half
    Case("forest2001_k31", "forest", (2001, 2001), 31, row=154, bucket=68),
    Case("forest2001_k32", "forest", (2001, 2001), 32, row=142, bucket=64),
    Case("forest2001_k33", "forest", (2001, 2001), 33, row=150, bucket=64),
    Case("forest2001_k48", "forest", (2001, 2001), 48, row=170, bucket=63),
    Case("forest2001_k64", "forest", (2001, 2001), 64, row=160, bucket=71),
    # n <= k: neighbour lists with empty places
    Case("sheet10_k20", "sheet", (10, 10), 20, row=86, bucket=36),
    Case("sheet20_k20", "sheet", (20, 20), 20, row=90, bucket=36),
    Case("sheet21_k20", "sheet", (21, 21), 20, row=88, bucket=30),
    Case("sheet65_k64", "sheet", (65, 65), 64, row=108, bucket=48),
)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
LONGEST_ROWS = tuple(c.name for c in sorted(CASES, key=lambda c: -c.row)[:3])
PUSH_ALL_CASES = ("hub70_s0_c0_k32", "hub180_s0_c90_k64", "forest2001_k64")

# the segmented call: every cloud has more than SEG_K points; at SEG_MOLL the clouds' own mollification
# lengths differ in the first digits
SEG_K, SEG_MOLL = 32, 1e-3


@functools.lru_cache(maxsize=None)
def segments():
    """[hub(70), forest(801), two-centre hub(40)] moved to the nodes of the batch's own lattice
    (skeletonize._lattice_offsets): the coordinates that the segmented call is given."""
    from pyqsm_amd.geometry import skeletonize as sk
    pts = [hub(70), forest(801, 801), two_centre_hub(40, 0, 0.05)]
    return tuple(frozen(p + o) for p, o in zip(pts, sk._lattice_offsets(pts)))


@functools.lru_cache(maxsize=None)
def _oracle_laplacian(key, k, moll):
    P = segments()[key[1]] if key[0] == "segment" else _CLOUDS[key[0]](*key[1:])
    L, mass = oracle.point_cloud_laplacian(P, k, moll)
    L.sort_indices()
    for a in (L.indptr, L.indices, L.data):
        a.setflags(write=False)
    return L, frozen(mass)


@functools.lru_cache(maxsize=None)
def _oracle_counts(key, k, moll):
    bucket, rows = oracle.point_cloud_laplacian_counts(_CLOUDS[key[0]](*key[1:]), k, moll)
    return frozen(bucket), frozen(rows)


def expected(case):
    """(L scipy CSR, mass) of the oracle, computed once per case; read-only."""
    return _oracle_laplacian((case.cloud,) + case.args, case.k, MOLL)


def expected_segment(j):
    return _oracle_laplacian(("segment", j), SEG_K, SEG_MOLL)


def counts(case):
    """(edge-bucket lengths, row contributions) of the oracle's build, once per case."""
    return _oracle_counts((case.cloud,) + case.args, case.k, MOLL)


def pattern(L):
    return L.indptr.tobytes() + L.indices.tobytes()


def differences(got, want, bound=1e-9):
    """One device result ((indptr, indices, data), mass) against the oracle's (L, mass): the list of what
    differs (empty: equal) and the two measured relative differences. The pattern must be the oracle's,
    data within `bound` x max |L|, mass within `bound` x max mass, and L equal to its transpose to the
    bit."""
    from scipy.sparse import csr_matrix
    (indptr, indices, data), mass = got
    L0, mass0 = want
    n = L0.shape[0]
    bad = []
    if not np.array_equal(indptr, L0.indptr):
        bad.append("indptr differs")
    if not np.array_equal(indices, L0.indices):
        bad.append("indices differ")
    if bad:
        return bad, float("nan"), float("nan")
    d_data = float(np.abs(data - L0.data).max() / np.abs(L0.data).max())
    d_mass = float(np.abs(mass - mass0).max() / mass0.max())
    if not d_data <= bound:
        bad.append(f"data differs by {d_data:.2e} of the largest entry")
    if not d_mass <= bound:
        bad.append(f"mass differs by {d_mass:.2e} of the largest mass")
    L = csr_matrix((data, indices, indptr), shape=(n, n))
    asym = abs(L - L.T)
    if asym.nnz and asym.max() != 0.0:
        bad.append(f"L - L.T reaches {asym.max():.2e}")
    return bad, d_data, d_mass


def off_diagonal(csr):
    indptr, indices, data = csr
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    return data[indices != rows]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main(device=0):
    """Every case of the table on the device against the oracle, one line each with the digest of the
    values; stops at the first difference. Returns the exit status. (A child process of
    tests/test_gpu_laplacian_classes.py runs this under PYQSM_LAP_ROWS=0, which is read once per
    process.)"""
    from pyqsm_amd import _lib, hip
    _lib.require_gpu(device)
    for case in CASES:
        got = hip.pc_laplacian(case.points, case.k, MOLL, device=device)
        bad, d_data, d_mass = differences(got, expected(case))
        if bad:
            print(f"{case.name}: MISMATCH: {'; '.join(bad)}", flush=True)
            return 1
        print(f"{case.name}: equal to the oracle, data {d_data:.1e} mass {d_mass:.1e} sha256 {digest(got[0][2])}",
              flush=True)
        print(f"    off-diagonal values sha256 {digest(off_diagonal(got[0]))}", flush=True)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())


