"""The aggregation multigrid of pyqsm_amd/csrc/amg.hip restated in NumPy / SciPy fp64, and the
systems of tests/test_amg_host.py and tests/test_gpu_amg.py.

``build(indptr, indices, vals, dense_max)`` repeats amg_build from the level-0 values of B on:
strength graph, MIS-2 roots by hashed priorities, the two joining passes, member lists, Galerkin
rows, diag and the l1 dinv, with the kernel's stop rules. Every sum is taken in the kernel's order
(``np.add.at`` adds one element after the other, in index order), so the arrays are the device's
bit for bit; only ``dinv`` passes through a division. ``ap_table`` restates k_ap_count / k_ap_fill.

``cycle(H, b, dtype)`` is the V(1,1) cycle as a linear map on [n, k] blocks of right-hand sides:
``np.float64`` is the reference, ``np.float32`` the same formulas on the fp32 roundings the kernels
use (valsf, dinvf, the a_ij * dinv_j products of k_entry_cols); the coarsest inverse stays fp64
there too, as in k_dense_solve / k_dense_mv. Plain NumPy; nothing here touches the library.
"""
import functools

import numpy as np
import scipy.sparse as sp

THETA = 0.08
ROW_CAP = 64
MAX_LEVELS = 24
COARSE_MAX = 96          # host Cholesky inverse at or below
DENSE_MAX = 1024         # device inverse at or below (PYQSM_AMG_DENSE_MAX, clamped to [96, 1024])
TAIL_SWEEPS = 8
FUSED_TAIL_MAX_ROWS = 3072
UNDECIDED, IN, OUT = 0, 1, 2
INF = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---- level construction -----------------------------------------------------------------------------

def rows_of(indptr):
    return np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))


def priority(i):
    """k_mis's hash of the point index: uint32 arithmetic that wraps, (h >> 1) above i + 1."""
    i = np.asarray(i, dtype=np.uint64)
    m = np.uint64(0xFFFFFFFF)
    h = (i * np.uint64(0x9E3779B1)) & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return ((h >> np.uint64(1)) << np.uint64(32)) | ((i + np.uint64(1)) & m)


def strong(indptr, indices, vals, diag):
    """Per stored entry: j != i and a_ij^2 >= theta^2 a_ii a_jj, the products taken left to right."""
    r = rows_of(indptr)
    return (indices != r) & (vals * vals >= ((THETA * THETA) * diag[r]) * diag[indices])


def diag_l1(indptr, indices, vals):
    """k_diag_l1: a_ii and 1 / sum_j |a_ij|, the sum taken in CSR order."""
    n = len(indptr) - 1
    r = rows_of(indptr)
    s = np.zeros(n)
    np.add.at(s, r, np.abs(vals))
    d = np.zeros(n)
    on = indices == r
    d[r[on]] = vals[on]
    with np.errstate(divide="ignore"):
        dinv = np.where(s > 0.0, 1.0 / s, 1.0)
    return d, dinv


def _nbr_max(key, r, c, n):
    out = key.copy()
    np.maximum.at(out, r, key[c])
    return out


def aggregate(indptr, indices, vals, diag):
    """(agg, mptr, members, nc, roots): k_mis_init, rounds of k_mis_max twice + k_mis_update, root numbers by
    prefix sum, k_agg1 and k_agg2 (the largest id wins), members ascending. nc = 0: no root at all."""
    n = len(indptr) - 1
    s = strong(indptr, indices, vals, diag)
    r, c = rows_of(indptr)[s], indices[s].astype(np.int64)
    has = np.zeros(n, bool)
    has[r] = True
    state = np.where(has, UNDECIDED, OUT)
    key = np.where(has, priority(np.arange(n)), np.uint64(0))
    while (state == UNDECIDED).any():
        t2 = _nbr_max(_nbr_max(key, r, c, n), r, c, n)
        und = state == UNDECIDED
        root = und & (t2 == key)
        out = und & ~root & (t2 == INF)
        state[root], key[root] = IN, INF
        state[out], key[out] = OUT, np.uint64(0)
    is_root = state == IN
    ids = np.cumsum(is_root) - is_root
    nc = int(is_root.sum())
    if nc == 0:
        return None, None, None, 0, is_root
    agg1 = np.where(is_root, ids, -1)
    to_root = is_root[c] & ~is_root[r]
    np.maximum.at(agg1, r[to_root], ids[c[to_root]])
    agg = agg1.copy()
    late = agg1[r] < 0
    np.maximum.at(agg, r[late], agg1[c[late]])
    mem = np.argsort(agg, kind="stable")
    mem = mem[agg[mem] >= 0]
    mptr = np.concatenate([[0], np.cumsum(np.bincount(agg[agg >= 0], minlength=nc))])
    return agg.astype(np.int32), mptr.astype(np.int32), mem.astype(np.int32), nc, is_root


def galerkin(indptr, indices, vals, agg, nc):
    """k_galerkin_rows + k_rows_to_csr: row I adds the entries (agg[j], a_ij) of its members in
    ascending order, entries in CSR order, columns without an aggregate skipped; the row is sorted by
    coarse column and every sum runs in that order of arrival; an entry below the diagonal then takes
    the sum of its mirror entry (the two add the same numbers in different orders). Returns None when a
    row would have more than ROW_CAP columns."""
    r = rows_of(indptr)
    I, J = agg[r].astype(np.int64), agg[indices].astype(np.int64)
    keep = (I >= 0) & (J >= 0)
    I, J, v = I[keep], J[keep], vals[keep]          # (row-major = members ascending, entries in order)
    keys, slot = np.unique(I * nc + J, return_inverse=True)
    cvals = np.zeros(len(keys))
    np.add.at(cvals, slot, v)
    cnt = np.bincount(keys // nc, minlength=nc)
    if cnt.max() > ROW_CAP:
        return None
    cptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    KI, KJ = keys // nc, keys % nc
    low = np.flatnonzero(KJ < KI)                   # below the diagonal: the sum of the row above it
    at = np.searchsorted(keys, KJ[low] * nc + KI[low])
    ok = (at < len(keys)) & (keys[np.minimum(at, len(keys) - 1)] == KJ[low] * nc + KI[low])
    cvals[low[ok]] = cvals[at[ok]]
    return cptr, KJ.astype(np.int32), cvals


def ap_table(indptr, indices, vals, agg):
    """k_ap_count / k_ap_fill: per row the distinct aggregates of its columns in order of first
    occurrence, each with the fp32 sum of its entries in CSR order."""
    valsf, aggcol = vals.astype(np.float32), agg[indices]
    ptr, idx, val = [0], [], []
    for i in range(len(indptr) - 1):
        seen = {}
        for q in range(indptr[i], indptr[i + 1]):
            a = aggcol[q]
            if a < 0:
                continue
            if a not in seen:
                seen[a] = len(idx)
                idx.append(a)
                val.append(np.float32(0.0))
            val[seen[a]] = np.float32(val[seen[a]] + valsf[q])
        ptr.append(len(idx))
    return np.array(ptr, np.int32), np.array(idx, np.int32), np.array(val, np.float32)


def build(indptr, indices, vals, dense_max=DENSE_MAX):
    """amg_build from level 0's CSR values of B. Returns {"levels": [...], "stop": reason, "coarse":
    "host" / "device" / "sweeps"}; stop is "dense" (n <= dense_max), "none" (no root), "ratio"
    (nc > 0.8 n), "cap" (a Galerkin row above ROW_CAP) or "levels"."""
    dense_max = max(COARSE_MAX, min(int(dense_max), DENSE_MAX))
    d, dinv = diag_l1(indptr, indices, vals)
    lv = [dict(n=len(indptr) - 1, indptr=np.asarray(indptr, np.int32), indices=np.asarray(indices, np.int32),
               vals=np.asarray(vals, np.float64), diag=d, dinv=dinv, agg=None, mptr=None, members=None)]
    stop = "levels"
    for _ in range(MAX_LEVELS):
        F = lv[-1]
        if F["n"] <= dense_max:
            stop = "dense"
            break
        agg, mptr, mem, nc, roots = aggregate(F["indptr"], F["indices"], F["vals"], F["diag"])
        if nc <= 0 or nc > 0.8 * F["n"]:
            stop = "none" if nc <= 0 else "ratio"
            break
        C = galerkin(F["indptr"], F["indices"], F["vals"], agg, nc)
        if C is None:
            stop = "cap"
            break
        F.update(agg=agg, mptr=mptr, members=mem, roots=roots)
        d, dinv = diag_l1(*C)
        lv.append(dict(n=nc, indptr=C[0], indices=C[1], vals=C[2], diag=d, dinv=dinv, agg=None, mptr=None,
                       members=None))
    last = lv[-1]["n"]
    coarse = "sweeps" if len(lv) < 2 or last > dense_max else ("host" if last <= COARSE_MAX else "device")
    return {"levels": lv, "stop": stop, "coarse": coarse}


def make_b(indptr, indices, lvals, cw, wh):
    """k_make_b in fp64 without a fused multiply-add: cw_i L_ij, plus wh_i on the diagonal."""
    r = rows_of(indptr)
    return cw[r] * lvals + np.where(indices == r, wh[r], 0.0)


def csr(L):
    return sp.csr_matrix((L["vals"], L["indices"], L["indptr"]), shape=(L["n"], L["n"]))


def prolongation(L, nc):
    on = np.flatnonzero(L["agg"] >= 0)
    return sp.csr_matrix((np.ones(len(on)), (on, L["agg"][on])), shape=(L["n"], nc))


# ---- the cycle -------------------------------------------------------------------------------------

def _operators(H, dtype):
    """Per level and number format: A, A Dinv (k_entry_cols' products), dinv, P, A P (k_ap_fill's sums)."""
    key = ("ops", np.dtype(dtype).name)
    if key not in H:
        ops = []
        for l, L in enumerate(H["levels"]):
            v, di = L["vals"].astype(dtype), L["dinv"].astype(dtype)
            shape = (L["n"], L["n"])
            A = sp.csr_matrix((v, L["indices"], L["indptr"]), shape=shape)
            AD = sp.csr_matrix((v * di[L["indices"]], L["indices"], L["indptr"]), shape=shape)
            P = AP = None
            if L["agg"] is not None:
                nc = H["levels"][l + 1]["n"]
                P = prolongation(L, nc).astype(dtype)
                if "ap" not in L:
                    L["ap"] = ap_table(L["indptr"], L["indices"], L["vals"], L["agg"])
                ptr, idx, val = L["ap"]
                AP = sp.csr_matrix((val, idx, ptr), shape=(L["n"], nc)) if dtype == np.float32 else (A @ P).tocsr()
            ops.append((A, AD, di[:, None], P, AP))
        H[key] = ops
    return H[key]


def coarse_inverse(H):
    if "inv" not in H:
        H["inv"] = np.linalg.inv(csr(H["levels"][-1]).toarray())
    return H["inv"]


def cycle(H, b, dtype=np.float64, level=0, ap=False):
    """One V(1,1) cycle on b [n, k] (k_down, k_restrict, the coarsest solve, k_up; ap: the upward step
    in k_up_ap's form, b - A y = r - (A P) xc with the residual of the downward step)."""
    ops = _operators(H, dtype)
    A, AD, di, P, AP = ops[level]
    b = np.asarray(b, dtype=dtype)
    if level == len(ops) - 1:
        if H["coarse"] != "sweeps":                 # fp64 inverse and accumulation, whatever the cycle's format
            return (coarse_inverse(H) @ b.astype(np.float64)).astype(dtype)
        x = di * b                                   # k_scale, then TAIL_SWEEPS of sweep_row
        for _ in range(TAIL_SWEEPS):
            x = x + di * (b - A @ x)
        return x
    x = di * b
    r = b - AD @ b
    xc = cycle(H, P.T @ r, dtype, level + 1, ap)
    y = x + P @ xc                                   # rows with agg = -1 get no correction
    return y + di * ((r - AP @ xc) if ap else (b - A @ y))


def cycle_matrix(H, level=0):
    """The fp64 cycle assembled from explicit P, Dinv and A matrices (dense)."""
    L = H["levels"][level]
    A, n = csr(L).toarray(), L["n"]
    S = np.diag(L["dinv"])
    if level == len(H["levels"]) - 1:
        if H["coarse"] != "sweeps":
            return np.linalg.inv(A)
        X = S.copy()
        for _ in range(TAIL_SWEEPS):
            X = X + S @ (np.eye(n) - A @ X)
        return X
    P = prolongation(L, H["levels"][level + 1]["n"]).toarray()
    Y = S + P @ cycle_matrix(H, level + 1) @ P.T @ (np.eye(n) - A @ S)
    return Y + S @ (np.eye(n) - A @ Y)


def d32(H, b, ap=False):
    """(fp64 cycle of b, what fp32 rounding alone costs: max |cycle_f32 - cycle_f64| / max |cycle_f64|)
    for one block of right-hand sides [n, k]; ap: the fp32 cycle takes its upward step as k_up_ap does."""
    x64 = cycle(H, b, np.float64)
    x32 = cycle(H, np.asarray(b, np.float32), np.float32, ap=ap)
    return x64, float(np.abs(x32.astype(np.float64) - x64).max() / np.abs(x64).max())


# ---- the systems -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def forest_system(n):
    """Cases A (n = 1500) and B (n = 6000): the rough system of tests/test_gpu_lbc.py."""
    import oracle
    from pyqsm_amd import synth
    P = synth.forest(n, seed=3)
    L, M = oracle.point_cloud_laplacian(P, 12, 1e-6)
    L, M = L.tocsr(), np.asarray(M)
    L.sort_indices()
    cw = np.full(n, 3e3 * np.sqrt(M.mean()))
    wh = 3.0 * np.sqrt(M.mean() / M) ** np.random.default_rng(0).uniform(0.5, 1.5, n)
    return L, cw, wh


def _laplacian(n, i, j, w):
    W = sp.coo_matrix((np.concatenate([w, w]), (np.concatenate([i, j]), np.concatenate([j, i]))), shape=(n, n)).tocsr()
    L = (sp.diags(np.asarray(W.sum(axis=1)).ravel()) - W).tocsr()
    L.sort_indices()
    return L


def _blocks(nb, rng):
    """nb complete cliques of 4 nodes, edge weights uniform in [0.5, 2]."""
    pi, pj = np.triu_indices(4, 1)
    base = 4 * np.arange(nb)[:, None]
    return (base + pi).ravel(), (base + pj).ravel(), rng.uniform(0.5, 2.0, nb * len(pi))


@functools.lru_cache(maxsize=None)
def clique_system(nb, seed=1):
    """Cases C (nb = 150) and D (nb = 3100): cliques coupled to cliques +1 and +7 by edges of weight
    1e-2; the second coarsening finds no strong edge."""
    rng = np.random.default_rng(seed)
    i, j, w = _blocks(nb, rng)
    k = np.arange(nb)
    ci = np.concatenate([4 * k + rng.integers(0, 4, nb), 4 * k + rng.integers(0, 4, nb)])
    cj = np.concatenate([4 * ((k + 1) % nb) + rng.integers(0, 4, nb), 4 * ((k + 7) % nb) + rng.integers(0, 4, nb)])
    n = 4 * nb
    L = _laplacian(n, np.concatenate([i, ci]), np.concatenate([j, cj]), np.concatenate([w, np.full(2 * nb, 1e-2)]))
    return L, np.ones(n), rng.uniform(0.25, 0.75, n)


@functools.lru_cache(maxsize=None)
def chord_system(nb=3100, seed=2, weak=1e-3, n_chords=420):
    """Case E: blocks of 4 nodes joined as a path by weak edges, plus random chords between blocks that
    are strong enough to be followed on level 1 only: most level-1 rows have no strong neighbour and are
    not represented on level 2 (empty rows of P)."""
    rng = np.random.default_rng(seed)
    i, j, w = _blocks(nb, rng)
    k = np.arange(nb - 1)
    pi, pj = 4 * k + rng.integers(0, 4, nb - 1), 4 * (k + 1) + rng.integers(0, 4, nb - 1)
    a = rng.integers(0, nb, n_chords)
    b = (a + rng.integers(2, nb - 2, n_chords)) % nb
    ci, cj = 4 * a + rng.integers(0, 4, n_chords), 4 * b + rng.integers(0, 4, n_chords)
    n = 4 * nb
    L = _laplacian(n, np.concatenate([i, pi, ci]), np.concatenate([j, pj, cj]),
                   np.concatenate([w, np.full(nb - 1, weak), np.full(n_chords, 0.3)]))
    return L, np.ones(n), rng.uniform(0.25, 0.75, n)


@functools.lru_cache(maxsize=None)
def hub_region_system(chains=30, seed=0):
    """Case F: cliques of 4 nodes (weights in [1, 2], wh in [0.01, 0.03]) whose couplings are weak on
    level 0 and strong on level 1, so that every clique becomes one level-1 row: three hub cliques
    joined to each other (4 edges of 0.3 a pair), each carrying `chains` chains of two cliques (0.2 to
    the hub, 0.05 along the chain). A hub row has chains + 3 columns on level 1; on level 2 the three
    merge into one aggregate whose row would have more than ROW_CAP columns."""
    rng = np.random.default_rng(seed)
    nb = 3 + 6 * chains
    pi, pj = np.triu_indices(4, 1)
    base = 4 * np.arange(nb)[:, None]
    i, j, w = [(base + pi).ravel()], [(base + pj).ravel()], [rng.uniform(1.0, 2.0, nb * len(pi))]
    t = np.arange(4)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        i.append(4 * a + t), j.append(4 * b + t), w.append(np.full(4, 0.3))
    first = 3 + 2 * np.arange(3 * chains)                      # chain q: cliques first[q], first[q] + 1
    hub = np.arange(3 * chains) % 3
    i.append(4 * hub + (np.arange(3 * chains) // 3) % 4), j.append(4 * first + rng.integers(0, 4, 3 * chains))
    w.append(np.full(3 * chains, 0.2))
    i.append(4 * first + rng.integers(0, 4, 3 * chains)), j.append(4 * (first + 1) + rng.integers(0, 4, 3 * chains))
    w.append(np.full(3 * chains, 0.05))
    n = 4 * nb
    # clique q is level-1 row q; the first hub clique takes the row with the largest priority, so it
    # is a root on level 1 and the other two hubs join it
    perm = np.arange(nb)
    top = int(np.argmax(priority(np.arange(nb))))
    perm[0], perm[top] = top, 0
    i, j = np.concatenate(i), np.concatenate(j)
    L = _laplacian(n, 4 * perm[i // 4] + i % 4, 4 * perm[j // 4] + j % 4, np.concatenate(w))
    return L, np.ones(n), rng.uniform(0.01, 0.03, n)


@functools.lru_cache(maxsize=None)
def hub_system(spokes=80, length=13, seed=5):
    """Case G: a hub with more than ROW_CAP spokes, every spoke a chain of `length` nodes (1041 rows,
    above every dense limit): the first Galerkin product overflows the row cap."""
    rng = np.random.default_rng(seed)
    s = 1 + length * np.arange(spokes)
    i = np.concatenate([np.zeros(spokes, np.int64)] + [s + t for t in range(length - 1)])
    j = np.concatenate([s] + [s + t + 1 for t in range(length - 1)])
    n = 1 + length * spokes
    L = _laplacian(n, i, j, rng.uniform(0.5, 2.0, len(i)))
    return L, np.ones(n), rng.uniform(0.25, 0.75, n)


def level0(system):
    L, cw, wh = system
    return L.indptr.astype(np.int32), L.indices.astype(np.int32), make_b(L.indptr, L.indices, L.data, cw, wh)


def right_hand_sides(n, seed=7):
    """A dozen Gaussian [n, 3] blocks, then one scaled by 1e-6 and one by 1e6."""
    g = np.random.default_rng(seed).normal(size=(14, n, 3))
    g[12] *= 1e-6
    g[13] *= 1e6
    return g


# name -> (system, PYQSM_AMG_DENSE_MAX or None, level sizes, stop rule, coarsest solve)
CASES = {
    "A": (lambda: forest_system(1500), None, [1500, 265], "dense", "device"),
    "A96": (lambda: forest_system(1500), 96, [1500, 265, 53], "dense", "host"),
    "B": (lambda: forest_system(6000), None, [6000, 1009], "dense", "device"),
    "B96": (lambda: forest_system(6000), 96, [6000, 1009, 158, 25], "dense", "host"),
    "C96": (lambda: clique_system(150), 96, [600, 150], "none", "sweeps"),
    "D": (lambda: clique_system(3100), None, [12400, 3100], "none", "sweeps"),
    "E": (lambda: chord_system(), None, [12400, 3095, 325], "dense", "device"),
    "F96": (lambda: hub_region_system(34), 96, [828, 207], "cap", "sweeps"),
    "G": (lambda: hub_system(), None, [1041], "cap", "sweeps"),
}


@functools.lru_cache(maxsize=None)
def restated(name):
    """The hierarchy of a case from the restated level-0 values (shared; the operators it caches are
    the only thing added to it)."""
    system, dmax, _, _, _ = CASES[name]
    return build(*level0(system()), DENSE_MAX if dmax is None else dmax)
