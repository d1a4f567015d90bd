"""NumPy statement of the epiphyte split's contract (include/pyqsm_hip.h, "epiphyte split"): the order
statistics of a per-row key, NumPy's linear percentile with its ``_lerp``, the three-way labelling of
``identify_epiphytes`` and the k-means++ / Lloyd of ``pyqsm_kmeans_pp``, with exactly the orders of
addition the header states (chunk sum, the seeding's sampling scan, the tie rules). The GPU tests
compare bit for bit against this file; tests/test_epiphyte_host.py holds it to NumPy and to
scikit-learn's recorded results."""
import numpy as np

CHUNK = 256


# ---------------------------------------------------------------- sums

def chunk_totals(v):
    """Chunk sums along the last axis: 256 values per chunk (zero padded), groups of four
    ((v0 + v1) + v2) + v3, the 64 group sums pairwise (neighbours first). [..., nch]."""
    v = np.asarray(v, dtype=np.float64)
    n = v.shape[-1]
    nch = max(1, -(-n // CHUNK))
    w = np.zeros(v.shape[:-1] + (nch * CHUNK,))
    w[..., :n] = v
    w = w.reshape(v.shape[:-1] + (nch, 64, 4))
    s = ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]
    while s.shape[-1] > 1:
        s = s[..., 0::2] + s[..., 1::2]
    return s[..., 0]


def seq_sum(t):
    """The values of the last axis added one at a time from 0.0."""
    t = np.asarray(t, dtype=np.float64)
    zero = np.zeros(t.shape[:-1] + (1,))
    return np.add.accumulate(np.concatenate([zero, t], axis=-1), axis=-1)[..., -1]


def chunk_sum(v):
    return seq_sum(chunk_totals(v))


# ---------------------------------------------------------------- selection and percentiles

def keys_of(v, key):
    """The keys of the rows of ``v`` [n] or [n,3]: column ``key``, or for 'norm'
    sqrt(((x*x) + (y*y)) + (z*z)). -0.0 is keyed as +0.0; a NaN anywhere is refused."""
    v = np.asarray(v, dtype=np.float64)
    if np.isnan(v).any():
        raise ValueError("the values hold a NaN")
    if v.ndim == 1:
        v = v[:, None]
    if key == "norm":
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        k = np.sqrt(((x * x) + (y * y)) + (z * z))
    else:
        k = v[:, key]
    return k + 0.0           # -0.0 + 0.0 = +0.0


def select(v, ranks, key=0):
    """np.sort(keys)[ranks]; a negative rank is an unused slot and gives 0.0."""
    ranks = np.asarray(ranks, dtype=np.int64)
    s = np.sort(keys_of(v, key))
    out = np.zeros(len(ranks))
    out[ranks >= 0] = s[ranks[ranks >= 0]]
    return out


def percentile_ranks(m, q):
    """(lo, hi, t) of NumPy's linear rule: virtual index (m - 1) * (q / 100)."""
    v = (m - 1) * (q / 100.0)
    lo = np.floor(v)
    return int(lo), min(int(lo) + 1, m - 1), float(v - lo)


def lerp(a, b, t):
    """NumPy's _lerp on scalars."""
    diff = b - a
    out = a + diff * t
    if t >= 0.5:
        out = b - diff * (1 - t)
    if t == 0:
        out = a
    return np.float64(out)


def percentile(keys, q):
    """np.percentile(keys, q) from the two neighbouring order statistics."""
    s = np.sort(np.asarray(keys, dtype=np.float64) + 0.0)
    lo, hi, t = percentile_ranks(len(s), q)
    return lerp(s[lo], s[hi], t)


def shift_components(shift, q_mag=65, q_z=60):
    """(labels uint8 [n], thresholds [2], counts [3]): 0 = norm not above P(q_mag); among the rows
    above it 1 = z above P(q_z) of their z (leaf), 2 = the rest (epiphyte)."""
    shift = np.asarray(shift, dtype=np.float64)
    labels = np.zeros(len(shift), np.uint8)
    thr = np.full(2, np.nan)
    if len(shift):
        mag = keys_of(shift, "norm")
        thr[0] = percentile(mag, q_mag)
        high = mag > thr[0]
        if high.any():
            z = shift[high, 2]
            thr[1] = percentile(z, q_z)
            labels[high] = np.where(z > thr[1], 1, 2)
    return labels, thr, np.bincount(labels, minlength=3).astype(np.int64)


# ---------------------------------------------------------------- k-means++ and Lloyd

def trials(k):
    return 2 + int(np.log(k))


def d2(x, c):
    """((dx*dx) + dy*dy) + dz*dz of the rows of x [n,d] to c [d], always direct."""
    dx = x[:, 0] - c[0]
    out = dx * dx
    for j in range(1, x.shape[1]):
        dj = x[:, j] - c[j]
        out = out + dj * dj
    return out


def nearest(x, cen):
    """The nearest centre of every row, ties to the lowest."""
    return np.argmin(np.stack([d2(x, c) for c in cen]), axis=0).astype(np.int32)   # argmin: first minimum


def sample(closest, r):
    """The first point at which the running sum of ``closest`` reaches ``r``, the sum taken as the
    header states: chunk totals in order, then the chunk's values from the total before it."""
    n = len(closest)
    cum = np.add.accumulate(np.concatenate([[0.0], chunk_totals(closest)]))   # cum[b] = total before chunk b
    reach = np.nonzero(cum[1:] >= r)[0]
    b = int(reach[0]) if len(reach) else len(cum) - 2
    seg = closest[b * CHUNK:min((b + 1) * CHUNK, n)]
    run = np.add.accumulate(np.concatenate([[cum[b]], seg]))[1:]
    hit = np.nonzero(run >= r)[0]
    return b * CHUNK + (int(hit[0]) if len(hit) else len(seg) - 1)


def seed_centres(xc, k, first, u):
    """Greedy k-means++ on centred points: the chosen indices [k]."""
    T = trials(k)
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    assert len(u) == (k - 1) * T
    seeds = [int(first)]
    closest = None
    for c in range(1, k):
        dd = d2(xc, xc[seeds[-1]])
        closest = dd if closest is None else np.where(dd < closest, dd, closest)
        pot = chunk_sum(closest)
        cands = [sample(closest, u[(c - 1) * T + t] * pot) for t in range(T)]
        pots = []
        for i in cands:
            dd = d2(xc, xc[i])
            pots.append(chunk_sum(np.where(dd < closest, dd, closest)))
        seeds.append(cands[int(np.argmin(pots))])      # argmin: ties to the earlier trial
    return np.array(seeds, np.int64)


class Result:
    pass


def kmeans_pp(x, k, first, u, max_iter=300, tol=1e-4):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    n, d = x.shape
    if not (1 <= k <= 64 and n >= k):
        raise ValueError("n >= k, 1 <= k <= 64")
    mu = np.array([chunk_sum(x[:, j]) / n for j in range(d)])
    xc = x - mu
    var = [chunk_sum(xc[:, j] * xc[:, j]) / n for j in range(d)]
    s = var[0]
    for j in range(1, d):
        s = s + var[j]
    tol_abs = tol * (s / d)
    seeds = seed_centres(xc, k, first, u)
    cen = xc[seeds].copy()
    labels_old = np.full(n, -1, np.int32)
    it, strict = 0, False
    while True:
        labels = nearest(xc, cen)
        member = labels[None, :] == np.arange(k)[:, None]                  # [k, n]
        cnt = member.sum(axis=1)
        new = cen.copy()
        for j in range(d):
            sums = seq_sum(chunk_totals(np.where(member, xc[None, :, j], 0.0)))
            new[cnt > 0, j] = sums[cnt > 0] / cnt[cnt > 0]                 # an empty centre keeps its place
        e = new - cen
        shift = 0.0
        for c in range(k):
            dd = e[c, 0] * e[c, 0]
            for j in range(1, d):
                dd = dd + e[c, j] * e[c, j]
            shift = shift + dd
        cen = new
        it += 1
        if np.array_equal(labels, labels_old):
            strict = True
            break
        if shift <= tol_abs or it >= max_iter:
            break
        labels_old = labels
    if not strict:
        labels = nearest(xc, cen)
    dist = np.zeros(n)
    for c in range(k):
        dist = np.where(labels == c, d2(xc, cen[c]), dist)
    out = Result()
    out.labels, out.centres, out.inertia, out.n_iter = labels, cen + mu, float(chunk_sum(dist)), it
    out.n_empty = int(k - len(np.unique(labels)))
    out.seeds, out.tol_abs = seeds, tol_abs
    return out


def kmeans_pp_plain(x, k, first, u, max_iter=300, tol=1e-4):
    """The same algorithm with NumPy's ordinary sums (means, np.cumsum sampling): what the goldens were
    first checked with; kept to show that the chunk order changes no label on general-position clouds."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    n, d = x.shape
    mu = x.mean(axis=0)
    xc = x - mu
    tol_abs = tol * np.mean(np.var(xc, axis=0))
    T = trials(k)
    seeds, closest = [int(first)], None
    for c in range(1, k):
        dd = d2(xc, xc[seeds[-1]])
        closest = dd if closest is None else np.minimum(closest, dd)
        pot = closest.sum()
        cands = np.clip(np.searchsorted(np.cumsum(closest), np.asarray(u[(c - 1) * T:c * T]) * pot), None, n - 1)
        pots = [np.minimum(closest, d2(xc, xc[i])).sum() for i in cands]
        seeds.append(int(cands[int(np.argmin(pots))]))
    cen = xc[seeds].copy()
    labels_old = np.full(n, -1, np.int32)
    it, strict = 0, False
    while True:
        labels = nearest(xc, cen)
        new = cen.copy()
        for c in range(k):
            if (labels == c).any():
                new[c] = xc[labels == c].mean(axis=0)
        shift = ((new - cen) ** 2).sum()
        cen = new
        it += 1
        if np.array_equal(labels, labels_old):
            strict = True
            break
        if shift <= tol_abs or it >= max_iter:
            break
        labels_old = labels
    if not strict:
        labels = nearest(xc, cen)
    out = Result()
    out.labels, out.centres, out.n_iter, out.seeds = labels, cen + mu, it, np.array(seeds, np.int64)
    out.inertia = float(sum(d2(xc[labels == c], cen[c]).sum() for c in range(k)))
    return out


# ---------------------------------------------------------------- inputs

def cloud(kind, n, d=3, seed=0):
    """Test clouds: 'tree' a noisy trunk with branches, 'box' uniform, 'blobs' eight Gaussians,
    'lattice' points snapped to a coarse grid (many exact distance ties), 'few' five distinct
    positions repeated."""
    rng = np.random.default_rng(seed)
    if kind == "tree":
        t = rng.uniform(0, 1, n)
        branch = rng.integers(0, 6, n)
        ang = branch * (np.pi / 3)
        out = np.stack([np.where(branch > 0, t * 4 * np.cos(ang), 0.0), np.where(branch > 0, t * 4 * np.sin(ang), 0.0),
                        np.where(branch > 0, 3 + branch + 2 * t, 12 * t)], axis=1)
        out = out + rng.normal(0, 0.15, (n, 3))
    elif kind == "box":
        out = rng.uniform(-10, 10, (n, 3))
    elif kind == "blobs":
        out = rng.normal(0, 1, (n, 3)) + rng.uniform(-12, 12, (8, 3))[rng.integers(0, 8, n)]
    elif kind == "lattice":
        out = rng.integers(0, 6, (n, 3)).astype(np.float64) * 0.5
    elif kind == "few":
        out = rng.normal(0, 3, (5, 3))[rng.integers(0, 5, n)]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(out[:, :d])


def shift_field(n, seed=0):
    """A first-contraction-step shift field: small for a wood-like half, larger and mostly downward
    for the rest, with exact zeros, signed zeros and repeated rows."""
    rng = np.random.default_rng(seed)
    s = rng.normal(0, 0.02, (n, 3))
    big = rng.random(n) < 0.5
    s[big] += rng.normal(0, 0.3, (int(big.sum()), 3)) + np.array([0, 0, -0.1])
    s[::97] = 0.0
    s[5::193, 2] = -0.0
    s[3::211] = s[3]
    return s
