"""numpy restatement of octfusion_amd.normals: the exact k-nearest-neighbour search with its fp32 distance and tie rule,
the per-point PCA and the flood-march-vote orientation, plus the analytic test shapes.  Written from the contract in
include/ofx.h (the block of csrc/ofx_normals.hip), not from the kernels: the search is a full sort, the eigenvectors
come from numpy.linalg.eigh, the flood is a breadth-first search."""
import numpy as np

F = np.float32


# ------------------------------------------------------------------------------------------------------------ kNN
def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, for float32 arrays with a * b + c >= 0: the product of two fp32 numbers is
    exact in float64; the float64 sum is moved to the odd neighbour when it was inexact (TwoSum gives the error), and
    a value rounded to odd at 53 bits rounds to 24 bits as the exact value does."""
    pr = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), pr.shape)
    t = pr + c
    bb = t - pr
    err = (pr - (t - bb)) + (c - bb)
    even = (t.view(np.int64) & 1) == 0
    t = np.where((err != 0) & even, np.nextafter(t, np.where(err > 0, np.inf, -np.inf)), t)
    return t.astype(F)


def dist2(q, t):
    """[m, n] float32: fma(dz, dz, fma(dy, dy, dx * dx)) from direct fp32 differences of q [m, 3] and t [n, 3]."""
    q, t = np.asarray(q, F), np.asarray(t, F)
    dx, dy, dz = (q[:, None, a] - t[None, :, a] for a in range(3))
    return fma32(dz, dz, fma32(dy, dy, dx * dx))


def knn(p, k, chunk=512):
    """(idx [n, k] int32, d2 [n, k] float32): per point the k smallest (d2, idx) over the whole cloud, itself
    included, by a full stable sort on d2 (equal d2 keep ascending idx); (-1, +inf) where the cloud has fewer than k."""
    p = np.asarray(p, F).reshape(-1, 3)
    n = p.shape[0]
    idx = np.full((n, k), -1, np.int32)
    d2 = np.full((n, k), np.inf, F)
    m = min(n, k)
    for i in range(0, n, chunk):
        d = dist2(p[i:i + chunk], p)
        order = np.argsort(d, axis=1, kind='stable')[:, :m]
        idx[i:i + chunk, :m] = order
        d2[i:i + chunk, :m] = np.take_along_axis(d, order, 1)
    return idx, d2


# ------------------------------------------------------------------------------------------------------------ PCA
def pca(p, idx):
    """(normals [n, 3] float32, variation [n] float32, degenerate [n] bool, gap [n] float64) from the valid entries of
    each row of idx: float64 centroid and covariance (/ m) summed in neighbour order, numpy.linalg.eigh, the
    eigenvector of the smallest eigenvalue rounded once to float32 and signed so that its component of largest
    magnitude (lowest axis on ties) is positive; variation = max(l0, 0) / (l0 + l1 + l2).  Fewer than 3 neighbours or
    an eigenvalue sum that is not positive: zeros, degenerate.  gap = (l1 - l0) / l2, how well the normal is defined."""
    p = np.asarray(p, F).reshape(-1, 3)
    idx = np.asarray(idx)
    n, k = idx.shape
    valid = (idx >= 0) & (idx < n)
    m = valid.sum(1)
    P = p[np.where(valid, idx, 0)].astype(np.float64)
    s = np.zeros((n, 3))
    for j in range(k):
        s += np.where(valid[:, j, None], P[:, j], 0.0)
    c = s / np.maximum(m, 1)[:, None]
    cov = np.zeros((n, 3, 3))
    for j in range(k):
        d = np.where(valid[:, j, None], P[:, j] - c, 0.0)
        cov += d[:, :, None] * d[:, None, :]
    cov /= np.maximum(m, 1)[:, None, None]
    w, v = np.linalg.eigh(cov)
    tot = w.sum(1)
    degenerate = (m < 3) | ~(tot > 0)
    e = v[:, :, 0]
    e = (e / np.linalg.norm(e, axis=1, keepdims=True)).astype(F)
    lead = np.argmax(np.abs(e), axis=1)                      # the first maximum: lowest axis on ties
    flip = e[np.arange(n), lead] < 0
    e = np.where(flip[:, None], -e, e)
    safe = np.where(degenerate, 1.0, tot)
    var = (np.maximum(w[:, 0], 0.0) / safe).astype(F)
    gap = (w[:, 1] - w[:, 0]) / np.where(w[:, 2] > 0, w[:, 2], 1.0)
    e[degenerate] = 0
    var[degenerate] = 0
    return e, var, degenerate, gap


# --------------------------------------------------------------------------------------------------------- orient
def cube(p):
    """(lo [3], e) float32: the bounding cube centred on the box centre, side = the largest extent (1 without one)."""
    p = np.asarray(p, F).reshape(-1, 3)
    mn, mx = p.min(0), p.max(0)
    e = (mx - mn).max()
    if not e > 0:
        e = F(1)
    return (mn + mx) * F(0.5) - e * F(0.5), F(e)


def auto_grid(e, d2, k):
    """clamp(floor(e / mean distance to the neighbour of rank min(k, 16) - 1), 8, 128)."""
    r = np.sqrt(np.asarray(d2)[:, min(k, 16) - 1].astype(np.float64))
    r = r[np.isfinite(r)]
    if r.size == 0 or not r.mean() > 0:
        return 8
    return int(min(max(np.floor(float(e) / r.mean()), 8), 128))


def _coord(x, lo, h):
    return np.floor((x - lo) / h)                            # float32 throughout: two roundings and a floor


def exterior(p, lo, e, G):
    """(occupied, exterior) bool [G + 2] ^ 3 indexed [x, y, z]."""
    p = np.asarray(p, F).reshape(-1, 3)
    lo, h = np.asarray(lo, F), F(e) / F(G)
    D = G + 2
    c = (np.clip(_coord(p, lo, h), 0, G - 1) + 1).astype(np.int64)
    occ = np.zeros((D + 2,) * 3, bool)                       # one more layer all round, so that no index leaves
    steps = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    for dx, dy, dz in steps:
        occ[c[:, 0] + 1 + dx, c[:, 1] + 1 + dy, c[:, 2] + 1 + dz] = True
    wall = np.ones_like(occ)
    wall[1:-1, 1:-1, 1:-1] = False
    border = np.zeros_like(occ)
    border[1:-1, 1:-1, 1:-1] = True
    border[2:-2, 2:-2, 2:-2] = False
    blocked = (occ | wall).ravel()
    seen = (border & ~occ).ravel().copy()
    front = np.flatnonzero(seen)
    S = D + 2
    offs = np.array([S * S, -S * S, S, -S, 1, -1])
    while front.size:
        nb = (front[:, None] + offs[None, :]).ravel()
        nb = np.unique(nb[~blocked[nb] & ~seen[nb]])
        seen[nb] = True
        front = nb
    ext = seen.reshape(occ.shape)[1:-1, 1:-1, 1:-1]
    return occ[1:-1, 1:-1, 1:-1], ext


def _first_exit(p, d, lo, h, G, ext, steps2):
    n = p.shape[0]
    first = np.full(n, steps2 + 1, np.int64)
    h2 = h * F(0.5)
    for s in range(1, steps2 + 1):
        t = F(s) * h2
        q = p + t * d
        v = _coord(q, lo, h)
        inside = ((v >= -1) & (v <= G)).all(1)
        cell = np.where(inside[:, None], v + 1, 0).astype(np.int64)
        hit = ~inside | ext[cell[:, 0], cell[:, 1], cell[:, 2]]
        first = np.where(hit & (first == steps2 + 1), s, first)
    return first


def orient(p, nrm, idx, lo, e, G, steps=8, rounds=3):
    """(out [n, 3] float32, sign [n] int8, counts dict) of the flood, march and votes on one cloud."""
    p, nrm = np.asarray(p, F).reshape(-1, 3), np.asarray(nrm, F).reshape(-1, 3)
    idx = np.asarray(idx)
    n, k = idx.shape
    lo, h = np.asarray(lo, F), F(e) / F(G)
    _, ext = exterior(p, lo, e, G)
    a = _first_exit(p, nrm, lo, h, G, ext, 2 * steps)
    b = _first_exit(p, -nrm, lo, h, G, ext, 2 * steps)
    marched = np.where(a < b, 1, np.where(b < a, -1, 0)).astype(np.int8)
    s = marched.copy()
    valid = (idx >= 0) & (idx < n)
    nb = np.where(valid, idx, 0)
    N = nrm.astype(np.float64)
    for _ in range(rounds):
        d = np.zeros(n)
        for j in range(k):                                   # in neighbour order, one term at a time
            t = nb[:, j]
            dot = (N[t, 0] * N[:, 0] + N[t, 1] * N[:, 1]) + N[t, 2] * N[:, 2]
            d = d + np.where(valid[:, j], s[t].astype(np.float64) * dot, 0.0)
        s = np.where(d > 0, 1, np.where(d < 0, -1, s)).astype(np.int8)
    out = np.where((s == -1)[:, None], -nrm, nrm)
    counts = {'undecided_after_march': int((marched == 0).sum()),
              'flipped_by_vote': int(((marched != 0) & (s == -marched)).sum()),
              'undecided': int((s == 0).sum()), 'degenerate': int((nrm == 0).all(1).sum())}
    return out, s, counts


def estimate(p, k=16, steps=8, rounds=3, grid=None):
    """The whole pipeline on one cloud: (oriented normals, unoriented normals, sign, G, counts)."""
    idx, d2 = knn(p, k)
    nrm, _, _, _ = pca(p, idx)
    lo, e = cube(p)
    G = auto_grid(e, d2, k) if grid is None else grid
    out, s, counts = orient(p, nrm, idx, lo, e, G, steps, rounds)
    return out, nrm, s, G, counts


# --------------------------------------------------------------------------------------------------------- shapes
def sphere(n, r=0.7, centre=(0.0, 0.0, 0.0), seed=0):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * r + np.asarray(centre)).astype(F), d.astype(F)


def torus(n, R=0.55, r=0.2, seed=0):
    """Uniform by area: the density along the tube angle v is proportional to R + r cos v (rejection)."""
    rng = np.random.default_rng(seed)
    v = np.empty(0)
    while v.size < n:
        c = rng.uniform(0, 2 * np.pi, 2 * n)
        keep = rng.uniform(0, R + r, 2 * n) < R + r * np.cos(c)
        v = np.concatenate([v, c[keep]])
    v = v[:n]
    u = rng.uniform(0, 2 * np.pi, n)
    nn = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], 1)
    pp = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], 1)
    return pp.astype(F), nn.astype(F)


def two_spheres(n_each, seed=0):
    a = sphere(n_each, 0.3, (-0.5, 0.0, 0.0), seed)
    b = sphere(n_each, 0.3, (0.5, 0.1, 0.0), seed + 1000)
    return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])


def box(n, half=(0.8, 0.5, 0.3), centre=(0.0, 0.0, 0.0), seed=0, rng=None):
    """Uniform by area on the surface of an axis-aligned box; the normal is the face's."""
    rng = np.random.default_rng(seed) if rng is None else rng
    half = np.asarray(half, np.float64)
    area = np.array([half[1] * half[2], half[0] * half[2], half[0] * half[1]])
    ax = rng.choice(3, n, p=area / area.sum())
    sg = rng.integers(0, 2, n) * 2.0 - 1.0
    pp = rng.uniform(-1, 1, (n, 3)) * half
    nn = np.zeros((n, 3))
    pp[np.arange(n), ax] = sg * half[ax]
    nn[np.arange(n), ax] = sg
    return (pp + np.asarray(centre)).astype(F), nn.astype(F)


def plate(n, seed=0):
    return box(n, (0.4, 0.3, 0.025), seed=seed)


CHAIR = [((0.0, 0.0, 0.0), (0.4, 0.4, 0.05)),                              # seat
         ((0.0, -0.35, 0.35), (0.4, 0.05, 0.35)),                          # back
         ((0.3, 0.3, -0.3), (0.06, 0.06, 0.3)), ((-0.3, 0.3, -0.3), (0.06, 0.06, 0.3)),
         ((0.3, -0.3, -0.3), (0.06, 0.06, 0.3)), ((-0.3, -0.3, -0.3), (0.06, 0.06, 0.3))]    # legs, 0.12 wide


def chair(n, seed=0):
    """A union of overlapping boxes: samples of each box's surface that lie strictly inside another box are dropped."""
    rng = np.random.default_rng(seed)
    areas = np.array([8 * (h[0] * h[1] + h[1] * h[2] + h[0] * h[2]) for _, h in CHAIR])
    P, N = np.empty((0, 3), F), np.empty((0, 3), F)
    while P.shape[0] < n:
        for j, (c, h) in enumerate(CHAIR):
            pp, nn = box(int(np.ceil(n * areas[j] / areas.sum())), h, c, rng=rng)
            keep = np.ones(len(pp), bool)
            for i, (c2, h2) in enumerate(CHAIR):
                if i != j:
                    keep &= ~(np.abs(pp.astype(np.float64) - np.asarray(c2)) < np.asarray(h2)).all(1)
            P, N = np.concatenate([P, pp[keep]]), np.concatenate([N, nn[keep]])
    sel = rng.permutation(P.shape[0])[:n]
    return P[sel], N[sel]


def lattice(n, seed=0, side=9):
    """n distinct points of an integer lattice, scaled by 1/8: differences, squares and sums are exact, ties abound."""
    rng = np.random.default_rng(seed)
    flat = rng.choice(side ** 3, n, replace=False)
    return (np.stack(np.unravel_index(flat, (side,) * 3), 1) / 8.0).astype(F)


def angle_deg(a, b):
    """Unoriented angle between unit vectors, in degrees."""
    d = np.abs((np.asarray(a, np.float64) * np.asarray(b, np.float64)).sum(1))
    return np.degrees(np.arccos(np.clip(d, 0.0, 1.0)))
