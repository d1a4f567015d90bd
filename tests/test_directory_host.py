"""The ranked cell directory's contract and both producer rules (tests/directory_restatement.py) on
every cloud of tests/test_gpu_dbscan_directory.py, without a GPU: the look-up through the words and
slots a producer leaves equals the dense count for every entry, no look-up reads a slot that nobody
wrote, and every cloud has the geometry its GPU test claims."""
import numpy as np
import pytest

from tests import directory_restatement as D

FULL = 1 << 22      # directories up to here are compared entry by entry, larger ones at the entries that matter


def _entries(pl):
    if pl.ncell <= FULL:
        return np.arange(pl.ncell + 1, dtype=np.int64)
    occ = np.unique(pl.cells)
    edges = np.arange(pl.nbk + 1, dtype=np.int64) << pl.bits
    rng = np.random.default_rng(0)
    c = np.concatenate([occ - 1, occ, occ + 1, occ + 2, edges - 1, edges, edges + 1, [0, pl.ncell],
                        rng.integers(0, pl.ncell + 1, 100_000)])
    return np.unique(c[(c >= 0) & (c <= pl.ncell)])


@pytest.mark.parametrize("name", list(D.CLOUDS))
def test_cloud_has_the_geometry_it_claims(name):
    D.claim(name)


@pytest.mark.parametrize("name", list(D.CLOUDS))
def test_bucket_rule_reproduces_the_dense_directory(name):
    pl = D.plan(name)
    n = len(pl.cells)
    bits, base, slots = D.from_buckets(pl.cells, pl.ncell, pl.bits)
    assert len(bits) == pl.nbk << (pl.bits - 5) and len(slots) == n + pl.nbk + 1
    c = _entries(pl)
    want = np.searchsorted(np.sort(pl.cells), c)
    got = D.lookup(bits, base, slots, c)
    assert np.array_equal(got, want)
    assert got[-1] == n and c[-1] == pl.ncell
    inside = c[c < pl.ncell]
    assert np.array_equal(D.occupied(bits, inside), np.isin(inside, pl.cells))
    # cells past ncell inside the last bucket have no bit
    past = np.arange(pl.ncell, pl.nbk << pl.bits, dtype=np.int64)
    assert not D.occupied(bits, past).any()


@pytest.mark.parametrize("name", [k for k in D.CLOUDS if D.plan(k).ncell <= FULL])
def test_word_rule_reproduces_the_dense_directory(name):
    pl = D.plan(name)
    start = D.dense(pl.cells, pl.ncell)
    bits, base, slots = D.from_dense(start, pl.ncell)
    assert len(slots) == len(pl.cells) + (pl.ncell >> 5) + 2
    c = np.arange(pl.ncell + 1, dtype=np.int64)
    assert np.array_equal(D.lookup(bits, base, slots, c), start)
    assert np.array_equal(D.occupied(bits, c[:-1]), start[1:] != start[:-1])


def test_word_rule_on_a_directory_of_one_bucket13_row():
    """The word rule where ncell is far from a multiple of 32 and most words are empty."""
    rng = np.random.default_rng(5)
    ncell = 100_003
    cells = rng.choice(ncell, 700)
    start = D.dense(cells, ncell)
    bits, base, slots = D.from_dense(start, ncell)
    assert np.array_equal(D.lookup(bits, base, slots, np.arange(ncell + 1)), start)
    for b in (12, 13):
        bits, base, slots = D.from_buckets(cells, ncell, b)
        assert np.array_equal(D.lookup(bits, base, slots, np.arange(ncell + 1)), start)
