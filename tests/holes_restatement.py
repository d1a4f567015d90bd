"""The hole-filling contract (include/pyqsm_hip.h) stated in NumPy and plain Python: twins,
successor, loops and their order, flags, the minimum-area table with its tie rule, the pre-order rows and
the statistics. Written from the contract's text, independent of csrc/holes_exact.hpp; the host tests
hold it against a brute force over all triangulations, the GPU tests hold the kernels against it bit for
bit. NumPy's elementwise products, differences and sqrt are IEEE operations without fusing, which is what
the contract's area formula asks for."""
from typing import NamedTuple

import numpy as np

FILL_MAX_LOOP = 128


class Fill(NamedTuple):
    ptr: np.ndarray         # int32 [n_loops + 1]
    verts: np.ndarray       # int32 [ptr[-1]]
    flags: np.ndarray       # uint8 [n_loops]
    area: np.ndarray        # float64 [n_loops]
    new_tris: np.ndarray    # int32 [n_new, 3]
    new_loop: np.ndarray    # int32 [n_new]
    stats: np.ndarray       # int64 [8]
    splits: list            # per loop: {(i, k): j} of the filled loops, None otherwise

    def loop(self, i):
        return self.verts[self.ptr[i]:self.ptr[i + 1]]


def _next(h):
    return h - 2 if h % 3 == 2 else h + 1


def twins(tris):
    """twin [3T]: the opposite half-edge on an edge of exactly two triangles that run opposite ways; -1 on
    an edge of one triangle; -2 on an edge of more than two, or of two that run the same way."""
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    nh = 3 * len(t)
    tail = t.reshape(-1)
    head = t[:, [1, 2, 0]].reshape(-1)
    key = (np.minimum(tail, head) << 32) | np.maximum(tail, head)
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    twin = np.full(nh, -2, np.int64)
    twin[cnt[inv] == 1] = -1
    order = np.argsort(inv, kind="stable")
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    two = start[cnt == 2]
    a, b = order[two], order[two + 1]
    opp = tail[a] != tail[b]
    twin[a[opp]] = b[opp]
    twin[b[opp]] = a[opp]
    return twin, tail, key


def successors(tris):
    """{h: succ(h) or None} over the boundary half-edges, by rotation about the head vertex."""
    twin, tail, key = twins(tris)
    fan = np.bincount(tail) if len(tail) else np.zeros(0, np.int64)
    succ = {}
    for h in np.nonzero(twin == -1)[0].tolist():
        g = _next(h)
        out = None
        for _ in range(int(fan[tail[g]])):
            if twin[g] == -1:
                out = g
                break
            if twin[g] < 0:
                break
            g = _next(int(twin[g]))
        succ[h] = out
    return succ, tail, key


def loops(tris):
    """[(v_0, h_0, [v_0 .. v_{L-1}])] ascending by (v_0, h_0), and the number of boundary half-edges."""
    succ, tail, key = successors(tris)
    state = {}                                  # h -> 'chain' | 'cycle'
    cycles = []
    for h0 in succ:
        if h0 in state:
            continue
        path, seen, h = [], set(), h0
        while h is not None and h not in state and h not in seen:
            seen.add(h)
            path.append(h)
            h = succ[h]
        if h is not None and h in seen:         # came back: succ is injective, so to the beginning
            assert h == h0
            cycles.append(path)
            for g in path:
                state[g] = "cycle"
        else:
            for g in path:
                state[g] = "chain"
    out = []
    for cyc in cycles:
        L = len(cyc)
        s = min(range(L), key=lambda r: (int(tail[cyc[r]]), cyc[r]))
        cyc = cyc[s:] + cyc[:s]
        verts = [0] * L
        for r, h in enumerate(cyc):
            verts[(L - r) % L] = int(tail[h])
        out.append((verts[0], cyc[0], verts))
    out.sort(key=lambda x: (x[0], x[1]))
    return out, len(succ), key


def area(pi, pj, pk):
    """A(i, j, k) for one p_i and arrays (or single rows) p_j, p_k."""
    u, v = pj - pi, pk - pi
    cx = u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1]
    cy = u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2]
    cz = u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]
    return 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)


def min_area_table(p):
    """(W [L,L], split {(i, k): j}) of the loop's points p f64 [L,3]."""
    p = np.asarray(p, np.float64)
    L = len(p)
    W = np.zeros((L, L))
    split = {}
    for d in range(2, L):
        for i in range(L - d):
            k = i + d
            js = np.arange(i + 1, k)
            w = (W[i, js] + W[js, k]) + area(p[i], p[js], p[k])
            best, bj = w[0], 0
            for m in range(1, len(w)):          # a later j only when strictly smaller
                if w[m] < best:
                    best, bj = w[m], m
            W[i, k] = best
            split[(i, k)] = int(js[bj])
    return W, split


def rows_of(L, split):
    """[(i, j, k)] in pre-order: emit(i, k), then emit(i, j), then emit(j, k)."""
    rows, stack = [], [(0, L - 1)]
    while stack:
        i, k = stack.pop()
        if k - i < 2:
            continue
        j = split[(i, k)]
        rows.append((i, j, k))
        stack.append((j, k))
        stack.append((i, j))
    return rows


def fill(tris, verts, max_edges=None):
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    cap = FILL_MAX_LOOP if max_edges is None or max_edges <= 0 else int(max_edges)
    assert cap <= FILL_MAX_LOOP
    lps, n_boundary, key = loops(t)
    edges = set(key.tolist())
    ptr, lv, flags, areas, new_tris, new_loop, splits = [0], [], [], [], [], [], []
    stats = np.zeros(8, np.int64)
    stats[0], stats[1] = n_boundary, len(lps)
    for l, (_, _, ring) in enumerate(lps):
        L = len(ring)
        lv += ring
        ptr.append(len(lv))
        f = (1 if len(set(ring)) < L else 0) | (2 if L > cap else 0)
        flags.append(f)
        stats[3] += f & 1
        stats[4] += (f >> 1) & 1
        if f:
            areas.append(0.0)
            splits.append(None)
            continue
        stats[2] += 1
        p = v[ring]
        W, split = min_area_table(p)
        areas.append(W[0, L - 1])
        splits.append(split)
        for q, (i, j, k) in enumerate(rows_of(L, split)):
            new_tris.append((ring[i], ring[j], ring[k]))
            new_loop.append(l)
            stats[6] += int(area(p[i], p[j], p[k]) == 0.0)
            if q > 0:
                a, b = ring[i], ring[k]
                stats[7] += int(((min(a, b) << 32) | max(a, b)) in edges)
    stats[5] = n_boundary - len(lv)
    return Fill(np.asarray(ptr, np.int32), np.asarray(lv, np.int32), np.asarray(flags, np.uint8),
                np.asarray(areas, np.float64), np.asarray(new_tris, np.int32).reshape(-1, 3),
                np.asarray(new_loop, np.int32), stats, splits)


def brute_force_min_area(p):
    """The least total area over ALL triangulations of the polygon p, each summed on its own (so the sums
    associate differently from the table's)."""
    p = np.asarray(p, np.float64)

    def tri(i, k):                              # every triangulation of i .. k as a list of triangles
        if k - i < 2:
            yield []
            return
        for j in range(i + 1, k):
            for left in tri(i, j):
                for right in tri(j, k):
                    yield [(i, j, k)] + left + right

    best, count = None, 0
    for ts in tri(0, len(p) - 1):
        total = sum(float(area(p[i], p[j], p[k])) for i, j, k in ts)
        count += 1
        if best is None or total < best:
            best = total
    return best, count


# ---------------------------------------------------------------- shapes the tests share

def icosphere(level=2):
    """(verts f64 [V,3], tris int [T,3]) of a closed, outward-oriented sphere."""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v), np.asarray(f, np.int64)


def grid_surface(nu, nv, wrap_u, wrap_v, point):
    """A quad grid split into triangles; `point(i, j)` gives a vertex. Wrapped axes close up."""
    cu, cv = (nu if wrap_u else nu + 1), (nv if wrap_v else nv + 1)
    verts = np.asarray([point(i, j) for i in range(cu) for j in range(cv)], np.float64)

    def idx(i, j):
        return (i % cu) * cv + (j % cv)
    tris = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            tris += [(a, b, c), (a, c, d)]
    return verts, np.asarray(tris, np.int64)


def torus(nu=24, nv=12, R=2.0, r=0.7):
    def pt(i, j):
        a, b = 2 * np.pi * i / nu, 2 * np.pi * j / nv
        return ((R + r * np.cos(b)) * np.cos(a), (R + r * np.cos(b)) * np.sin(a), r * np.sin(b))
    return grid_surface(nu, nv, True, True, pt)


def tube(L, rings=2, wobble=0.3, seed=0):
    """An open tube whose two rims are L-gons; z varies along each rim, so the patches are not planar."""
    rng = np.random.default_rng(seed + L)
    dz = wobble * rng.standard_normal((rings + 1, L))

    def pt(i, j):
        a = 2 * np.pi * i / L
        return (np.cos(a) * (1 + 0.1 * j), np.sin(a) * (1 + 0.1 * j), j + dz[j, i])
    return grid_surface(L, rings, True, False, pt)


def sheet_with_holes(n=120, seed=5):
    """A noisy n x n sheet with one to four neighbouring triangles removed every third cell: many short
    loops of 3 to 6 edges, and the sheet's own rim of 4 n."""
    rng = np.random.default_rng(seed)
    z = 0.2 * rng.standard_normal((n + 1, n + 1))
    verts, tris = grid_surface(n, n, False, False, lambda i, j: (i, j, z[i, j]))
    keep = np.ones(len(tris), bool)
    step = 3
    for ci in range(1, n - 2, step):
        for cj in range(1, n - 2, step):
            kind = int(rng.integers(0, 4))
            q = 2 * (ci * n + cj)
            if kind == 0:
                keep[q] = False                          # one triangle: L = 3
            elif kind == 1:
                keep[q] = keep[q + 1] = False            # a quad: L = 4
            elif kind == 2:
                keep[q] = keep[q + 1] = keep[q + 2] = False
            else:
                keep[q] = keep[q + 1] = keep[q + 2] = keep[q + 3] = False
    return verts, tris[keep]
