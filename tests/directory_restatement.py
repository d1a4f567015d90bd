"""DBSCAN's ranked cell directory (pyqsm_amd/csrc/grid.hpp: CellDir), restated on the CPU, and the
clouds of tests/test_gpu_dbscan_directory.py.

The contract: 32 consecutive cell ids share one word (bits, base); bit i says cell 32 w + i holds a
point; ``begin(c) = slots[base + popcount(bits below c's bit)]``, and for every 0 <= c <= ncell that is
the number of points in cells with id < c, what ``np.searchsorted(sorted cell ids, c)`` gives.

Two producers are restated: ``from_buckets`` is k_bk_sort's rule (a bucket of 2^bits cells owns the
slots from bstart[b] + b: the begins of its occupied cells in id order, then bstart[b + 1]) and
``from_dense`` is k_dir_from_dense's (the same per word of a dense start array). Slots nobody writes
are filled with a poison value, so a look-up that strays reads nonsense here as it would on the GPU.

Every cloud carries the claims its GPU test makes about it (which words and buckets are occupied, their
populations, ncell modulo 32 and 4096); ``claim(name)`` recomputes them from grid_restatement's plan.
Plain NumPy; nothing here touches the library.
"""
import functools

import numpy as np

from tests import grid_restatement as G

POISON = -77_777_777
EPS = 0.1
CELL = EPS * (1.0 + 2.0 ** -20)


# ---- the contract and its two producers --------------------------------------------------------------

def dense(cells, ncell):
    """start[0 .. ncell]: points in cells with id < c."""
    return np.searchsorted(np.sort(np.asarray(cells, np.int64)), np.arange(ncell + 1, dtype=np.int64)).astype(np.int64)


def _popcount_below(bits, i):
    """popcount(bits & ((1 << i) - 1)) for arrays of 32-bit words and bit numbers."""
    return _popcount64(bits.astype(np.uint64) & ((np.uint64(1) << i.astype(np.uint64)) - np.uint64(1)))


def _popcount64(m):
    m = m - ((m >> np.uint64(1)) & np.uint64(0x5555555555555555))
    m = (m & np.uint64(0x3333333333333333)) + ((m >> np.uint64(2)) & np.uint64(0x3333333333333333))
    m = (m + (m >> np.uint64(4))) & np.uint64(0x0F0F0F0F0F0F0F0F)
    return ((m * np.uint64(0x0101010101010101)) >> np.uint64(56)).astype(np.int64)


def lookup(bits, base, slots, c):
    """begin(c) for an array of cell ids, as the kernels evaluate it."""
    c = np.asarray(c, np.int64)
    w = c >> 5
    return slots[base[w] + _popcount_below(bits[w], c & 31)]


def occupied(bits, c):
    c = np.asarray(c, np.int64)
    return ((bits[c >> 5] >> (c & 31).astype(np.uint64)) & np.uint64(1)).astype(bool)


def from_buckets(cells, ncell, bits_per_bucket):
    """k_bk_sort: (bits[nwords], base[nwords], slots[n + nbk + 1]) with nwords = nbk << (bits - 5)."""
    cells = np.sort(np.asarray(cells, np.int64))
    n = len(cells)
    nbk = (ncell + (1 << bits_per_bucket)) >> bits_per_bucket
    wpb = 1 << (bits_per_bucket - 5)
    bstart = np.searchsorted(cells, np.arange(nbk + 1, dtype=np.int64) << bits_per_bucket)
    assert bstart[nbk] == n
    bits = np.zeros(nbk * wpb, np.uint64)
    base = np.zeros(nbk * wpb, np.int64)
    slots = np.full(n + nbk + 1, POISON, np.int64)
    occ, first = np.unique(cells, return_index=True)          # occupied cells in id order, their begins
    for b in range(nbk):
        sb = int(bstart[b]) + b
        lo, hi = np.searchsorted(occ, [b << bits_per_bucket, (b + 1) << bits_per_bucket])
        mine = occ[lo:hi]
        assert len(mine) <= bstart[b + 1] - bstart[b]         # no more occupied cells than points
        slots[sb:sb + len(mine)] = first[lo:hi]
        slots[sb + len(mine)] = bstart[b + 1]                 # closes the bucket's slots
        wi = mine >> 5
        np.bitwise_or.at(bits, wi, np.uint64(1) << (mine & 31).astype(np.uint64))
        w0 = b * wpb
        before = np.searchsorted(mine, (np.arange(wpb, dtype=np.int64) + w0) << 5)
        base[w0:w0 + wpb] = sb + before
    return bits, base, slots


def from_dense(start, ncell):
    """k_dir_from_dense: word w reads start[32 w .. 32 w + 32] (entries past ncell read as start[ncell])."""
    start = np.asarray(start, np.int64)
    n = int(start[ncell])
    nwords = (ncell >> 5) + 1
    idx = np.minimum(np.arange(nwords * 32 + 1, dtype=np.int64), ncell)
    s = start[idx]
    occ = (s[1:] != s[:-1]).reshape(nwords, 32)
    bits = (occ.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint64)
    base = s[:-1:32] + np.arange(nwords, dtype=np.int64)
    slots = np.full(n + nwords + 1, POISON, np.int64)
    rank = np.cumsum(occ, 1) - occ
    w, i = np.nonzero(occ)
    slots[base[w] + rank[w, i]] = s[w * 32 + i]
    slots[base + occ.sum(1)] = s[32::32]
    return bits, base, slots


# ---- the clouds ------------------------------------------------------------------------------------

def cell_id(dims, cx, cy, cz):
    return (cz * dims[1] + cy) * dims[0] + cx


def cells_cloud(dims, fill, seed):
    """A cloud whose DBSCAN grid at EPS has exactly `dims` cells (border included) and `fill[id]`
    points in interior cell `id`, plus one corner point each in the first and the last interior cell
    (they fix the box). Points sit between 0.2 and 0.8 of their cell's edge; fp32-representable."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    ids = np.repeat(np.fromiter(fill.keys(), np.int64, len(fill)), np.fromiter(fill.values(), np.int64, len(fill)))
    cx, cy, cz = ids % nx, (ids // nx) % ny, ids // (nx * ny)
    assert ((cx >= 1) & (cx <= nx - 2) & (cy >= 1) & (cy <= ny - 2) & (cz >= 1) & (cz <= nz - 2)).all(), "interior cells"
    P = (np.stack([cx, cy, cz], 1) - 1 + rng.uniform(0.2, 0.8, (len(ids), 3))) * CELL
    top = (np.asarray(dims, np.float64) - 2.5) * CELL
    P = np.concatenate([[[0.0, 0.0, 0.0]], P, [top]])
    return G._f32(P)


def _interior(dims):
    nx, ny, nz = dims
    c = np.arange(nx * ny * nz, dtype=np.int64)
    cx, cy, cz = c % nx, (c // nx) % ny, c // (nx * ny)
    return c[(cx >= 1) & (cx <= nx - 2) & (cy >= 1) & (cy <= ny - 2) & (cz >= 1) & (cz <= nz - 2)]


WORD_DIMS = (66, 7, 6)       # an interior row of 64 cells holds a whole aligned word, whatever the row
BUCKET_DIMS = (66, 34, 12)   # 26 928 cells: seven buckets of 4096
PATHS_DIMS = (66, 34, 14)    # 31 416 cells: eight buckets
END_DIMS = {"end_0": (16, 16, 16), "end_4095": (15, 13, 21)}   # ncell % 4096 == 0 (and % 32 == 0); == 4095 (% 32 == 31)


def _word_edges():
    dims = WORD_DIMS
    nx = dims[0]
    inner = set(_interior(dims).tolist())
    fill = {}
    # ids = 31 and = 0 (mod 32) side by side in x (a stencil run [row - 1, row + 2) around either straddles two words)
    pair = next(c for c in sorted(inner) if c % 32 == 31 and c + 1 in inner and c // nx == (c + 1) // nx and c > 600)
    fill[pair], fill[pair + 1] = 4, 5
    # a word with all 32 cells occupied
    full = next(w for w in range(pair // 32 + 4, 10_000) if all(32 * w + i in inner for i in range(32)))
    for i in range(32):
        fill[32 * full + i] = 1 + i % 3
    # a word with only bit 0 set, one with only bit 31 set
    only0 = next(w for w in range(full + 3, 10_000) if 32 * w in inner)
    fill[32 * only0] = 6
    only31 = next(w for w in range(only0 + 3, 10_000) if 32 * w + 31 in inner)
    fill[32 * only31 + 31] = 7
    return cells_cloud(dims, fill, 1), dict(pair=pair, full=full, only0=only0, only31=only31)


def _bucket_edges():
    dims = BUCKET_DIMS
    fill = {4095: 5, 4096: 6, 4094: 3, 4097: 2}      # the last cells of bucket 0, the first of bucket 1
    rng = np.random.default_rng(2)
    inner = _interior(dims)
    for c in rng.choice(inner[(inner >> 12) == 0], 12, replace=False):   # bucket 0: a dozen cells, most words empty
        fill[int(c)] = fill.get(int(c), 0) + 4
    for c in rng.choice(inner[(inner >> 12) == 6], 9, replace=False):    # after the empty buckets 2 .. 5
        fill[int(c)] = fill.get(int(c), 0) + 5
    return cells_cloud(dims, fill, 3), {}


def _producer_paths():
    """Buckets of 1, 63, 64, 65, 0, about 1500 and more than 6144 points (the last with a cell above 255) and 1."""
    dims = PATHS_DIMS
    rng = np.random.default_rng(4)
    inner = _interior(dims)
    fill = {}

    def put(b, m, ncells, big=0):
        mine = rng.choice(inner[(inner >> 12) == b], ncells, replace=False)
        per = np.full(ncells, (m - big) // ncells)
        per[: (m - big) - per.sum()] += 1
        for c, k in zip(mine, per):
            fill[int(c)] = int(k)
        if big:
            fill[int(mine[0])] += big
    put(1, 63, 20)
    put(2, 64, 9)
    put(3, 65, 30)
    put(5, 1500, 300)
    put(6, 6500, 60, big=300)
    return cells_cloud(dims, fill, 5), {}


def _end(name):
    dims = END_DIMS[name]
    rng = np.random.default_rng(sum(dims))
    inner = _interior(dims)
    fill = {int(c): int(k) for c, k in zip(rng.choice(inner, 40, replace=False), rng.integers(1, 9, 40))}
    last = cell_id(dims, dims[0] - 2, dims[1] - 2, dims[2] - 2)
    fill[last - 1] = 3                                  # beside the corner point in the last interior cell
    return cells_cloud(dims, fill, 6), {}


def _tiny(name):
    if name == "tiny_1":
        return np.array([[0.25, 0.5, 0.75]]), {}
    rng = np.random.default_rng(7)
    if name == "tiny_64":
        return G._f32(rng.uniform(0, 1, (64, 3)) * [0.9, 0.4, 0.2]), {}
    return G._f32(rng.uniform(0.01, 0.09, (200, 3))), {}   # tiny_onecell


def _doubled():
    """tests/test_gpu_dbscan_tail.py::test_doubled_cell_path, 800 groups (min_pts 2)."""
    rng = np.random.default_rng(36 + 800 + 2)
    centres = np.cumsum(rng.uniform(0.6, 2.0, 800) * EPS)[:, None] * [1.0, 1.0, 1.0]
    sizes = rng.integers(1, 6, 800)
    P = np.concatenate([c + rng.uniform(0, 0.3 * EPS, (s, 3)) for c, s in zip(centres, sizes)])
    return P[rng.permutation(len(P))], {}


BITS13_DIMS = (407, 407, 406)

# name -> (eps, min_pts, the directory is read out, a device plan can hit)
CLOUDS = {
    "word_edges": (EPS, 3, True, True),
    "bucket_edges": (EPS, 3, True, True),
    "producer_paths": (EPS, 10, True, True),
    "end_0": (EPS, 3, True, True),
    "end_4095": (EPS, 3, True, True),
    "bits13": (G.EPS, G.MIN_PTS, False, False),
    "compressed": (0.03, 4, True, False),
    "doubled": (EPS, 2, False, False),
    "tiny_1": (EPS, 1, True, True),
    "tiny_64": (EPS, 3, True, True),
    "tiny_onecell": (EPS, 10, True, True),
}


@functools.lru_cache(maxsize=None)
def cloud(name):
    """(points, facts the builder chose: word and cell numbers the claims name)."""
    if name == "word_edges":
        P, facts = _word_edges()
    elif name == "bucket_edges":
        P, facts = _bucket_edges()
    elif name == "producer_paths":
        P, facts = _producer_paths()
    elif name in END_DIMS:
        P, facts = _end(name)
    elif name == "bits13":
        P, facts = G.threshold_cloud(BITS13_DIMS), {}
    elif name == "compressed":
        P, facts = G.axis_mapped_cloud(), {}
    elif name == "doubled":
        P, facts = _doubled()
    else:
        P, facts = _tiny(name)
    P = np.ascontiguousarray(P, np.float64)
    P.setflags(write=False)
    return P, facts


@functools.lru_cache(maxsize=None)
def plan(name):
    return G.dbscan_plan(cloud(name)[0], CLOUDS[name][0])


def claim(name):
    """Asserts what the cloud's test says about it; returns the plan."""
    P, f = cloud(name)
    pl = plan(name)
    cells, ncell = pl.cells, pl.ncell
    cnt = np.bincount(cells, minlength=ncell + 1)
    bucket = np.bincount(cells >> pl.bits, minlength=pl.nbk)
    word = lambda w: cnt[32 * w:32 * w + 32]
    if name == "word_edges":
        assert pl.dims == WORD_DIMS and not pl.mapped and not pl.doubled
        a = f["pair"]
        assert a % 32 == 31 and cnt[a] > 0 and cnt[a + 1] > 0 and (a + 1) % pl.dims[0] not in (0, pl.dims[0] - 1)
        assert (a - 1) >> 5 != (a + 2) >> 5, "the run [row - 1, row + 2) around the pair straddles two words"
        assert (word(f["full"]) > 0).all()
        assert (word(f["only0"]) > 0).tolist() == [True] + [False] * 31
        assert (word(f["only31"]) > 0).tolist() == [False] * 31 + [True]
    elif name == "bucket_edges":
        assert pl.dims == BUCKET_DIMS and (pl.bits, pl.nbk) == (12, 7)
        assert cnt[4095] > 0 and cnt[4096] > 0 and 4095 // pl.dims[0] == 4096 // pl.dims[0], "neighbours in x"
        assert bucket[1] > 0 and (bucket[2:6] == 0).all() and bucket[6] > 0
        w0 = np.array([(word(w) > 0).any() for w in range(128)])
        assert w0.any() and (~w0).sum() > 64, "empty words inside an occupied bucket"
    elif name == "producer_paths":
        assert pl.dims == PATHS_DIMS and (pl.bits, pl.nbk) == (12, 8)
        assert bucket.tolist()[:6] == [1, 63, 64, 65, 0, 1500] and bucket[7] == 1
        assert bucket[6] > G.tile(12) and cnt[(np.arange(ncell + 1) >> 12) == 6].max() > G.BK_BIG
        assert cnt[(np.arange(ncell + 1) >> 12) != 6].max() <= G.BK_BIG
    elif name in END_DIMS:
        assert pl.dims == END_DIMS[name]
        want = {"end_0": (0, 0), "end_4095": (4095, 31)}[name]
        assert (ncell % 4096, ncell % 32) == want
        if name == "end_0":
            assert pl.nbk == ncell // 4096 + 1 and bucket[-1] == 0, "entry ncell alone in a last bucket without a point"
    elif name == "bits13":
        G.claim_threshold_cloud(P, BITS13_DIMS)
        assert pl.bits == 13
    elif name == "compressed":
        assert pl.mapped and not pl.doubled and ncell + 1 <= (1 << 25)
    elif name == "doubled":
        assert pl.doubled
    elif name == "tiny_1":
        assert len(P) == 1
    elif name == "tiny_64":
        assert len(P) == 64 and (cnt > 0).sum() > 8
    else:
        assert (cnt > 0).sum() == 1 and len(P) == 200
    return pl
