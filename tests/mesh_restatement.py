"""The mesh-check contract restated in NumPy int64 / float64: what
``pyqsm_mesh_topology`` and ``pyqsm_mesh_self_intersections`` must return, and the named small
meshes the tests use. Plain and slow on purpose: sorts, Python union-finds, and the tri-tri decision
vectorised over candidate pairs. ``tests/test_mesh_host.py`` pins it against independent routes
(SciPy's connected components, exact rationals)."""
from __future__ import annotations

import math

import numpy as np

MAX_EXTENT = 1 << 20


# ---------------------------------------------------------------- named meshes

def _mesh(verts, tris):
    return np.asarray(verts, dtype=np.float64).reshape(-1, 3), np.asarray(tris, dtype=np.int32).reshape(-1, 3)


def tetrahedron():
    return _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])


def octahedron():
    v = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    t = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    return _mesh(v, t)


def cube():
    """The 12-triangle unit cube, outward winding."""
    v = [[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)]
    t = [[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4],
         [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]]
    return _mesh(v, t)


def cube_flipped():
    """The cube with triangle 5 wound the other way."""
    v, t = cube()
    t = t.copy()
    t[5] = t[5][::-1]
    return v, t


def sheet(m: int):
    """An open m x m sheet of quads, two triangles each."""
    g = np.arange(m + 1)
    x, y = np.meshgrid(g, g, indexing="xy")
    v = np.stack([x.ravel(), y.ravel(), np.zeros(x.size)], axis=1)
    t = []
    for j in range(m):
        for i in range(m):
            a = j * (m + 1) + i
            b, c, d = a + 1, a + m + 2, a + m + 1
            t += [[a, b, c], [a, c, d]]
    return _mesh(v, t)


def moebius(n_quads: int = 16):
    """A strip of n quads closed with a half twist: edge-manifold with boundary, not orientable."""
    v, t = [], []
    for i in range(n_quads):
        ang = 2 * math.pi * i / n_quads
        for s in (-1, 1):
            r = 2 + 0.5 * s * math.cos(ang / 2)
            v.append([r * math.cos(ang), r * math.sin(ang), 0.5 * s * math.sin(ang / 2)])
    for i in range(n_quads):
        a, b = 2 * i, 2 * i + 1
        if i + 1 < n_quads:
            c, d = 2 * i + 2, 2 * i + 3
        else:                      # the seam: the two sides change places
            c, d = 1, 0
        t += [[a, c, b], [b, c, d]]
    return _mesh(v, t)


def two_tets_one_vertex():
    """Two tetrahedra that share vertex 0 and nothing else."""
    v, t = tetrahedron()
    v2 = -v[1:]
    t2 = t.copy()
    t2[t2 > 0] += 3
    return _mesh(np.concatenate([v, v2]), np.concatenate([t, t2]))


def three_on_an_edge():
    """Three triangles around the edge (0, 1)."""
    v = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 1], [0, -1, -1]]
    return _mesh(v, [[0, 1, 2], [0, 1, 3], [1, 0, 4]])


def many_tets(n: int = 300, seed: int = 5):
    """n separate tetrahedra, their 4 n triangles in shuffled order."""
    rng = np.random.default_rng(seed)
    v0, t0 = tetrahedron()
    verts = np.concatenate([v0 * rng.uniform(0.5, 2.0) + rng.uniform(-20, 20, 3) for _ in range(n)])
    tris = np.concatenate([t0 + 4 * k for k in range(n)])
    return _mesh(verts, tris[rng.permutation(len(tris))])


def shuffled_strip(n_tris: int = 5000, seed: int = 6):
    """One long strip of triangles in shuffled order (long union-find chains)."""
    rng = np.random.default_rng(seed)
    k = np.arange(n_tris + 2)
    verts = np.stack([(k // 2).astype(float), (k % 2).astype(float), 0.01 * np.sin(k)], axis=1)
    tris = np.stack([k[:-2], k[1:-1], k[2:]], axis=1)
    tris[1::2] = tris[1::2][:, ::-1]
    return _mesh(verts, tris[rng.permutation(n_tris)])


NAMED = {
    "tetrahedron": tetrahedron, "octahedron": octahedron, "cube": cube, "cube_flipped": cube_flipped,
    "sheet": lambda: sheet(7), "moebius": moebius, "two_tets_one_vertex": two_tets_one_vertex,
    "three_on_an_edge": three_on_an_edge, "many_tets": many_tets, "shuffled_strip": shuffled_strip,
}


# ---------------------------------------------------------------- topology

def _smallest_labels(n: int, links) -> np.ndarray:
    """The smallest member of every node's set after joining the (a, b) of ``links``."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in links:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(x) for x in range(n)], dtype=np.int64)


def triangle_areas(verts, tris) -> np.ndarray:
    v = np.asarray(verts, dtype=np.float64)
    t = np.asarray(tris)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    ux, uy, uz = (b - a).T
    vx, vy, vz = (c - a).T
    cx, cy, cz = uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
    return 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)


def half_edge_runs(tris):
    """(u, w, order, first, count): half-edge h = 3 t + k runs u[h] -> w[h]; ``order`` sorts them by
    (min, max, h); ``first`` / ``count`` give each run of equal (min, max) in ``order``."""
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    u = t.reshape(-1)
    w = t[:, [1, 2, 0]].reshape(-1)
    a, b = np.minimum(u, w), np.maximum(u, w)
    order = np.lexsort((np.arange(len(u)), b, a))
    sa, sb = a[order], b[order]
    head = np.ones(len(u), bool)
    head[1:] = (sa[1:] != sa[:-1]) | (sb[1:] != sb[:-1])
    first = np.nonzero(head)[0]
    count = np.diff(np.append(first, len(u)))
    return u, w, order, first, count


def topology(tris, n_verts: int, verts=None) -> dict:
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    nt = len(t)
    out = {"edges": np.zeros((0, 2), np.int32), "edge_count": np.zeros(0, np.int32),
           "edge_flags": np.zeros(0, np.uint8), "tri_cluster": np.zeros(0, np.int32),
           "cluster_n": np.zeros(0, np.int64), "cluster_area": None if verts is None else np.zeros(0),
           "vertex_flags": np.zeros(n_verts, np.uint8),
           "summary": np.array([0, 0, 0, 0, 0, 0, 1, n_verts], np.int64)}
    if nt == 0:
        return out
    u, w, order, first, count = half_edge_runs(t)
    h0 = order[first]
    edges = np.stack([np.minimum(u[h0], w[h0]), np.maximum(u[h0], w[h0])], axis=1)
    flags = np.where(count == 1, 1, 0) | np.where(count > 2, 2, 0)
    tri_links, corner_links, cover_links = [], [], []
    nxt = lambda h: 3 * (h // 3) + (h % 3 + 1) % 3
    for e in range(len(first)):
        f, n = first[e], count[e]
        a0 = order[f]
        for h in order[f + 1:f + n]:
            same = u[h] == u[a0]
            tri_links.append((a0 // 3, h // 3))
            corner_links.append((a0, h if same else nxt(h)))
            corner_links.append((nxt(a0), nxt(h) if same else h))
            if n == 2:
                if same:
                    flags[e] |= 4
                cover_links.append((2 * (a0 // 3), 2 * (h // 3) + (1 if same else 0)))
                cover_links.append((2 * (a0 // 3) + 1, 2 * (h // 3) + (0 if same else 1)))
    lab = _smallest_labels(nt, tri_links)
    roots = np.unique(lab)
    cl = np.searchsorted(roots, lab)
    corner = _smallest_labels(3 * nt, corner_links)
    fans = np.zeros(n_verts, np.int64)
    is_root = corner == np.arange(3 * nt)
    np.add.at(fans, u[is_root], 1)
    cover = _smallest_labels(2 * nt, cover_links)
    orientable = int(not (count > 2).any() and not (cover[0::2] == cover[1::2]).any())
    out.update(edges=edges.astype(np.int32), edge_count=count.astype(np.int32), edge_flags=flags.astype(np.uint8),
               tri_cluster=cl.astype(np.int32), cluster_n=np.bincount(cl, minlength=len(roots)).astype(np.int64),
               vertex_flags=(fans > 1).astype(np.uint8))
    if verts is not None:
        area = triangle_areas(verts, t)
        out["tri_area"] = area
        out["cluster_area"] = np.array([math.fsum(area[cl == c].tolist()) for c in range(len(roots))])
    out["summary"] = np.array([len(first), int((flags & 1).astype(bool).sum()), int((flags & 2).astype(bool).sum()),
                               int((flags & 4).astype(bool).sum()), int((fans > 1).sum()), len(roots), orientable,
                               int((fans == 0).sum())], np.int64)
    return out


def kept_clusters(cluster_n, cluster_area, top_n_clusters=10, min_cluster_area=None, max_cluster_area=None) -> list:
    """The clusters ``get_surface_clusters`` keeps, one at a time: with ``top_n_clusters``, a cluster
    stays when fewer than ``top_n_clusters`` clusters have MORE triangles than it (so ties at the
    last place all stay); with the area bounds, when its area lies inside them (closed)."""
    kept = []
    for c, (n, area) in enumerate(zip(cluster_n, cluster_area)):
        ok = True
        if top_n_clusters:
            ok = sum(1 for m in cluster_n if m > n) < top_n_clusters
        if min_cluster_area is not None and area < min_cluster_area:
            ok = False
        if max_cluster_area is not None and area > max_cluster_area:
            ok = False
        if ok:
            kept.append(c)
    return kept


# ---------------------------------------------------------------- the exact tri-tri decision

def _orient3d(a, b, c, d):
    u, v, w = b - a, c - a, d - a
    return (w[:, 0] * (u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]) + w[:, 1] * (u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2])
            + w[:, 2] * (u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]))


def _orient2d(a, b, c):
    return (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])


def _agree(a, b, c):
    pos = (a > 0) | (b > 0) | (c > 0)
    neg = (a < 0) | (b < 0) | (c < 0)
    return ~(pos & neg)


def _on_segment(a, b, c):
    return ((np.minimum(a[:, 0], b[:, 0]) <= c[:, 0]) & (c[:, 0] <= np.maximum(a[:, 0], b[:, 0]))
            & (np.minimum(a[:, 1], b[:, 1]) <= c[:, 1]) & (c[:, 1] <= np.maximum(a[:, 1], b[:, 1])))


def _seg_seg_2d(p, q, a, b):
    d1, d2 = np.sign(_orient2d(p, q, a)), np.sign(_orient2d(p, q, b))
    d3, d4 = np.sign(_orient2d(a, b, p)), np.sign(_orient2d(a, b, q))
    return ((d1 * d2 < 0) & (d3 * d4 < 0)) | ((d1 == 0) & _on_segment(p, q, a)) | ((d2 == 0) & _on_segment(p, q, b)) \
        | ((d3 == 0) & _on_segment(a, b, p)) | ((d4 == 0) & _on_segment(a, b, q))


def _in_tri_2d(p, t):
    return _agree(_orient2d(t[0], t[1], p), _orient2d(t[1], t[2], p), _orient2d(t[2], t[0], p))


_KEEP = np.array([[1, 2], [2, 0], [0, 1]])


def _drop(v, axis):
    return np.take_along_axis(v, _KEEP[axis], axis=1)


def normals(tri):
    return np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])


def degenerate(tri) -> np.ndarray:
    """The three lattice vertices are collinear or coincide. tri int64 [n,3,3]."""
    return ~normals(np.asarray(tri, dtype=np.int64)).any(axis=1)


def _seg_tri(p, q, t, axis):
    sp, sq = np.sign(_orient3d(t[:, 0], t[:, 1], t[:, 2], p)), np.sign(_orient3d(t[:, 0], t[:, 1], t[:, 2], q))
    p2, q2 = _drop(p, axis), _drop(q, axis)
    t2 = [_drop(t[:, k], axis) for k in range(3)]
    flat = _in_tri_2d(p2, t2) | _in_tri_2d(q2, t2) | _seg_seg_2d(p2, q2, t2[0], t2[1]) \
        | _seg_seg_2d(p2, q2, t2[1], t2[2]) | _seg_seg_2d(p2, q2, t2[2], t2[0])
    through = _agree(_orient3d(p, q, t[:, 0], t[:, 1]), _orient3d(p, q, t[:, 1], t[:, 2]),
                     _orient3d(p, q, t[:, 2], t[:, 0]))
    return np.where(sp * sq > 0, False, np.where((sp == 0) & (sq == 0), flat, through))


def tri_tri(a, b) -> np.ndarray:
    """Whether the closed triangles a[n] and b[n] (int64 [n,3,3], none degenerate) have a common
    point: some edge of one meets the other."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    axa, axb = np.abs(normals(a)).argmax(axis=1), np.abs(normals(b)).argmax(axis=1)
    hit = np.zeros(len(a), bool)
    for k in range(3):
        k1 = (k + 1) % 3
        hit |= _seg_tri(a[:, k], a[:, k1], b, axb)
        hit |= _seg_tri(b[:, k], b[:, k1], a, axa)
    return hit


def self_intersections(ijk, tris, chunk: int = 4_000_000):
    """(pairs int32 [n,2] ascending, tri_hit uint8 [T], stats int64 [6]) of the contract."""
    p = np.asarray(ijk, dtype=np.int64).reshape(-1, 3)
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    nt = len(t)
    stats = np.zeros(6, np.int64)
    stats[0] = nt * (nt - 1) // 2
    hit = np.zeros(nt, np.uint8)
    if nt == 0:
        return np.zeros((0, 2), np.int32), hit, stats
    if len(p) and (p.max(axis=0) - p.min(axis=0)).max() > MAX_EXTENT:
        raise ValueError("extent above 2^20")
    tri = p[t]
    lo, hi = tri.min(axis=1), tri.max(axis=1)
    deg = degenerate(tri)
    stats[3] = int(deg.sum())
    found = []
    rows = max(1, chunk // nt)
    for r0 in range(0, nt, rows):                    # box overlap of rows r0 .. against every column j > i
        r = np.arange(r0, min(r0 + rows, nt))
        ov = ((lo[r, None] <= hi[None]) & (lo[None] <= hi[r, None])).all(axis=2)
        ov &= np.arange(nt)[None] > r[:, None]
        i, j = np.nonzero(ov)
        i = i + r0
        stats[1] += len(i)
        shared = (t[i][:, :, None] == t[j][:, None, :]).any(axis=(1, 2))
        stats[2] += int(shared.sum())
        go = ~shared & ~deg[i] & ~deg[j]
        i, j = i[go], j[go]
        stats[4] += len(i)
        yes = tri_tri(tri[i], tri[j])
        found.append(np.stack([i[yes], j[yes]], axis=1))
    found = np.concatenate(found)
    found = found[np.lexsort((found[:, 1], found[:, 0]))]
    pairs = np.array(found, np.int32).reshape(-1, 2)
    hit[pairs.reshape(-1)] = 1
    stats[5] = len(pairs)
    return pairs, hit, stats
