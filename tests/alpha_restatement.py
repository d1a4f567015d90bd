"""The alpha-area contract on the CPU: the directed-edge rule of DESIGN.md §17, restated three ways.

Points lie on an integer lattice, A2 is the squared radius. For a directed edge a->b and a third
point p: e = b - a, u = p - a, D = cross(e, u), N = u.(u - e), t_p = N / D.
  tl = min t_p over D > 0 (left of the edge), tr = max t_p over D < 0 (right of it);
  D == 0 and N < 0: p lies strictly inside the segment and kills the edge;
  a->b is an edge of the Delaunay subdivision iff it is not killed and one side is empty or tr < tl;
  its left cell is kept iff |e|^2 (D^2 + N^2) <= 4 A2 D^2 at the minimising point (inclusive);
  a kept left cell adds cross(a, b) to twice the area; kept left and not kept right: boundary edge.
Coincident points are merged first: the lowest index takes part.

  brute(P, A2)              Python integers, every point against every edge, no grid
  local(P, A2)              the same rule over the candidates within 2 alpha of a, numpy
  delaunay_filtered(P, A2)  scipy.spatial.Delaunay plus the exact integer circumradius filter

Each returns (twice_area, boundary) with boundary the sorted list of (a, b) original indices;
delaunay_filtered orients its triangles itself. All results are cached: the inputs are built from
fixed seeds and shared by the host and the GPU tests.
"""
import math

import numpy as np

_cache = {}


def live_points(P):
    """Indices of the points that take part: the lowest index of every distinct coordinate pair."""
    P = np.asarray(P, dtype=np.int64).reshape(-1, 2)
    seen, keep = {}, []
    for i, (x, y) in enumerate(P.tolist()):
        if (x, y) not in seen:
            seen[(x, y)] = i
            keep.append(i)
    return np.asarray(keep, dtype=np.int64)


def _decide(e2, has_l, nl, dl, has_r, nr, dr, killed, A2):
    """(left cell kept and a->b an edge, right cell kept) from Python integers."""
    if killed:
        return False, False
    if has_l and has_r and not (nr * dl > nl * dr):   # tr < tl, with dr < 0 < dl
        return False, False
    kept_l = has_l and e2 * (dl * dl + nl * nl) <= 4 * A2 * dl * dl
    kept_r = has_r and e2 * (dr * dr + nr * nr) <= 4 * A2 * dr * dr
    return kept_l, kept_r


def brute(P, A2):
    P = np.asarray(P, dtype=np.int64).reshape(-1, 2)
    key = ("brute", P.tobytes(), int(A2))
    if key in _cache:
        return _cache[key]
    A2 = int(A2)
    live = live_points(P).tolist()
    pts = [(int(P[i, 0]), int(P[i, 1])) for i in live]
    twice, boundary = 0, []
    for ia, (ax, ay) in enumerate(pts):
        rel = [(x - ax, y - ay) for (x, y) in pts]
        for ib, (ex, ey) in enumerate(rel):
            e2 = ex * ex + ey * ey
            if ib == ia or e2 > 4 * A2:      # a cell with this edge has circumradius >= |e| / 2
                continue
            has_l = has_r = killed = False
            nl = dl = nr = dr = 0
            for (ux, uy) in rel:
                D = ex * uy - ey * ux
                N = ux * (ux - ex) + uy * (uy - ey)
                if D > 0:
                    if not has_l or N * dl < nl * D:
                        has_l, nl, dl = True, N, D
                elif D < 0:
                    if not has_r or N * dr > nr * D:
                        has_r, nr, dr = True, N, D
                elif N < 0:
                    killed = True
                    break
            kept_l, kept_r = _decide(e2, has_l, nl, dl, has_r, nr, dr, killed, A2)
            if kept_l:
                bx, by = pts[ib]
                twice += ax * by - ay * bx
                if not kept_r:
                    boundary.append((live[ia], live[ib]))
    out = (twice, sorted(boundary))
    _cache[key] = out
    return out


def _best(N, D, t, side):
    """Per row the column with the smallest (side > 0, over D > 0) or largest (side < 0, over D < 0)
    N / D, exactly: the floating-point quotients t give a guess, exact cross-multiplication corrects
    it until no column beats it. Returns (has, n, d) per row."""
    mask = (D > 0) if side > 0 else (D < 0)
    has = mask.any(axis=1)
    c = np.where(mask, t, np.inf).argmin(axis=1) if side > 0 else np.where(mask, t, -np.inf).argmax(axis=1)
    rows = np.arange(N.shape[0])
    while True:
        nc, dc = N[rows, c], D[rows, c]
        # side > 0: column p beats c iff N_p d_c < n_c D_p (both D > 0);
        # side < 0: iff N_p d_c > n_c D_p (both D < 0)
        diff = N * dc[:, None]
        diff -= nc[:, None] * D
        better = ((diff < 0) if side > 0 else (diff > 0))
        better &= mask
        better &= has[:, None]
        fix = better.any(axis=1)
        if not fix.any():
            return has, nc, dc
        c = np.where(fix, better.argmax(axis=1), c)


def local(P, A2):
    from scipy.spatial import cKDTree
    P = np.asarray(P, dtype=np.int64).reshape(-1, 2)
    key = ("local", P.tobytes(), int(A2))
    if key in _cache:
        return _cache[key]
    A2 = int(A2)
    live = live_points(P)
    Q = P[live]
    twice, boundary = 0, []
    if len(Q) >= 3:
        reach = math.isqrt(4 * A2) + 1
        near = cKDTree(Q.astype(np.float64)).query_ball_point(Q.astype(np.float64), reach * (1 + 1e-9) + 1e-6)
        for ia in range(len(Q)):
            cand = np.asarray(near[ia], dtype=np.int64)
            U = Q[cand] - Q[ia]                                  # [k, 2], a itself among them
            d2 = U[:, 0] * U[:, 0] + U[:, 1] * U[:, 1]
            sel = d2 <= 4 * A2                                   # exactly within 2 alpha
            cand, U, d2 = cand[sel], U[sel], d2[sel]
            bsel = cand != ia
            E, e2 = U[bsel], d2[bsel]
            if not len(E):
                continue
            big = int(np.abs(U).max()) * 2 + 1
            M = 2 * big * big                                    # |N|, |D| <= M
            if 2 * (4 * A2 + int(e2.max())) * M * M >= 2 ** 62:  # the products leave int64: Python ints
                U, E, e2 = U.astype(object), E.astype(object), e2.astype(object)
            ex, ey = E[:, 0][:, None], E[:, 1][:, None]
            ux, uy = U[:, 0][None, :], U[:, 1][None, :]
            D = ex * uy - ey * ux
            N = ux * (ux - ex) + uy * (uy - ey)
            killed = ((D == 0) & (N < 0)).any(axis=1)
            with np.errstate(divide="ignore", invalid="ignore"):
                t = N.astype(np.float64) / D.astype(np.float64)
            has_l, nl, dl = _best(N, D, t, +1)
            has_r, nr, dr = _best(N, D, t, -1)
            is_edge = ~killed & (~has_l | ~has_r | (nr * dl > nl * dr))
            kept_l = is_edge & has_l & (e2 * (dl * dl + nl * nl) <= 4 * A2 * dl * dl)
            kept_r = has_r & (e2 * (dr * dr + nr * nr) <= 4 * A2 * dr * dr)
            bi = cand[bsel]
            ax, ay = int(Q[ia, 0]), int(Q[ia, 1])
            for j in np.nonzero(kept_l.astype(bool))[0]:
                bx, by = int(Q[bi[j], 0]), int(Q[bi[j], 1])
                twice += ax * by - ay * bx
                if not kept_r[j]:
                    boundary.append((int(live[ia]), int(live[bi[j]])))
    out = (int(twice), sorted(boundary))
    _cache[key] = out
    return out


def delaunay_filtered(P, A2):
    from scipy.spatial import Delaunay
    P = np.asarray(P, dtype=np.int64).reshape(-1, 2)
    key = ("delaunay", P.tobytes(), int(A2))
    if key in _cache:
        return _cache[key]
    A2 = int(A2)
    live = live_points(P)
    Q = P[live]
    twice, kept = 0, set()
    if len(Q) >= 3:
        tri = Delaunay(Q.astype(np.float64)).simplices
        for (i, j, k) in tri.tolist():
            (ax, ay), (bx, by), (cx, cy) = (tuple(map(int, Q[v])) for v in (i, j, k))
            cr = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
            if cr == 0:
                continue
            if cr < 0:
                j, k, cr = k, j, -cr
                (bx, by), (cx, cy) = (cx, cy), (bx, by)
            la = (bx - ax) ** 2 + (by - ay) ** 2
            lb = (cx - bx) ** 2 + (cy - by) ** 2
            lc = (ax - cx) ** 2 + (ay - cy) ** 2
            if la * lb * lc <= 4 * A2 * cr * cr:       # R^2 = |ab|^2 |bc|^2 |ca|^2 / (4 cr^2) <= A2
                twice += cr
                kept.update(((i, j), (j, k), (k, i)))
    boundary = sorted((int(live[a]), int(live[b])) for (a, b) in kept if (b, a) not in kept)
    out = (int(twice), boundary)
    _cache[key] = out
    return out


def degrees_balanced(boundary):
    """Every vertex of a boundary list has as many outgoing as incoming edges."""
    out, inn = {}, {}
    for a, b in boundary:
        out[a] = out.get(a, 0) + 1
        inn[b] = inn.get(b, 0) + 1
    return out == inn


def loops(boundary):
    """The closed loops of a boundary in which every vertex has one outgoing edge: a list of
    (vertex list, twice the signed area of the loop)."""
    nxt = dict(boundary)
    assert len(nxt) == len(boundary)
    seen, res = set(), []
    for a0 in sorted(nxt):
        if a0 in seen:
            continue
        loop, a = [], a0
        while a not in seen:
            seen.add(a)
            loop.append(a)
            a = nxt[a]
        assert a == a0
        res.append(loop)
    return res


# ---------------------------------------------------------------- inputs

def random_points(n=150, size=400, seed=7):
    return np.random.default_rng(seed).integers(0, size, size=(n, 2)).astype(np.int32)


def holey_lattice(nx=12, ny=10, pitch=10, seed=11):
    """A lattice with 20 % of its nodes removed and ten stray points."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(nx) * pitch, np.arange(ny) * pitch, indexing="ij")
    nodes = np.stack([gx.ravel(), gy.ravel()], axis=1)
    nodes = nodes[rng.permutation(len(nodes))[: len(nodes) - len(nodes) // 5]]
    stray = rng.integers(0, (min(nx, ny) - 1) * pitch, size=(10, 2))
    return np.concatenate([nodes, stray]).astype(np.int32)


CIRCLE_65 = [(65, 0), (56, 33), (33, 56), (0, 65), (-33, 56), (-56, 33), (-65, 0), (-56, -33), (-33, -56),
             (0, -65), (33, -56), (56, -33)]


def cocircular(move=None):
    """Twelve exactly cocircular points (x^2 + y^2 = 65^2) scaled by 1000 and centred on
    (5e5, 5e5), plus three points outside the circle. move = (index, dx, dy) shifts one of them."""
    assert all(x * x + y * y == 65 * 65 for x, y in CIRCLE_65)
    pts = [(500000 + 1000 * x, 500000 + 1000 * y) for x, y in CIRCLE_65]
    pts += [(600000, 520000), (430000, 590000), (520000, 400000)]
    P = np.asarray(pts, dtype=np.int32)
    if move is not None:
        P[move[0]] += np.asarray(move[1:], dtype=np.int32)
    return P


def big_cloud(n=20000, size=4096, seed=3):
    return np.random.default_rng(seed).integers(0, size, size=(n, 2)).astype(np.int32)


def big_cloud_a2(n=20000, size=4096):
    """alpha of three mean spacings."""
    return int(9 * size * size // n)


def corners(per=40, box=1 << 20, span=1000, seed=5):
    """`per` points in each of two opposite corners of a box x box square."""
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, span, size=(per, 2))
    hi = box - rng.integers(0, span, size=(per, 2))
    return np.concatenate([lo, hi]).astype(np.int32)


def dense_cloud(n=2300, size=300, seed=13):
    """n distinct points in size^2: with alpha = size / 2 one grid cell holds them all, more than the
    2048 stencil points the edge kernel stages at a time and 72 slices of 32 points."""
    rng = np.random.default_rng(seed)
    flat = rng.choice(size * size, size=n, replace=False)
    return np.stack([flat // size, flat % size], axis=1).astype(np.int32)


def square_lattice(m=6, pitch=4):
    gx, gy = np.meshgrid(np.arange(m) * pitch, np.arange(m) * pitch, indexing="ij")
    return np.stack([gx.ravel(), gy.ravel()], axis=1).astype(np.int32)


def annulus(r_in=6, r_out=12, pitch=3):
    g = np.arange(-r_out, r_out + 1)
    gx, gy = np.meshgrid(g, g, indexing="ij")
    r2 = gx * gx + gy * gy
    sel = (r2 >= r_in * r_in) & (r2 <= r_out * r_out)
    return (np.stack([gx[sel], gy[sel]], axis=1) * pitch + r_out * pitch).astype(np.int32)


# The three small groups with an alpha that keeps nothing, one that keeps a part and one that keeps
# (nearly) everything: the largest A2 the device entry point accepts.
SMALL_GROUPS = {
    "random": (random_points, (0, 900, 1 << 40)),
    "lattice": (holey_lattice, (0, 50, 1 << 40)),
    "cocircular": (cocircular, (1000 ** 2, 65000 ** 2, 1 << 40)),
}
