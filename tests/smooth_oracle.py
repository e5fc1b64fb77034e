"""Float64 oracle of the mesh-graph contract (include/ofx.h, csrc/ofx_meshsmooth.hip): adjacency, vertex normals and
Laplacian / Taubin smoothing of ONE mesh.  numpy only, no project imports, and not the kernels' algorithm: ``np.lexsort``
and run lengths where the device radix-sorts keys and scans, ``np.add.at`` (which adds one element after the other, in
the order given) over pairs sorted in the contract's order where the device loops over a row.

Every expression is the header's own, operation by operation: numpy rounds every float64 operation on its own.
``tests/test_smooth_oracle.py`` pins this file to hand-written answers.
"""
import numpy as np

AREA, ANGLE, UNIFORM = 0, 1, 2                   # modes of vertex_normals
FIXED, SLIDE, FREE = 0, 1, 2                     # boundary rules of smooth
MODES = {'area': AREA, 'angle': ANGLE, 'uniform': UNIFORM}
BOUNDARY = {'fixed': FIXED, 'slide': SLIDE, 'free': FREE}
WEIGHTS = {'uniform': 0, 'cot': 1}


def _v32(V):
    return np.ascontiguousarray(np.asarray(V, np.float32).reshape(-1, 3))


def _faces(F):
    return np.asarray(F, np.int64).reshape(-1, 3)


def _cross(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                     u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)


def _dot(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def _len(x):
    return np.sqrt(_dot(x, x))


def refused(V, F):
    """The status word: a face index outside [0, V) or a non-finite vertex used by a face (any face)."""
    V, F = _v32(V), _faces(F)
    if ((F < 0) | (F >= len(V))).any():
        return True
    return not np.isfinite(V[F.reshape(-1)]).all()


def part(F):
    """Faces that take part: three different indices."""
    F = _faces(F)
    return (F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2])


def _pairs(F):
    """The directed pairs of the faces that take part, sorted by (vertex, neighbour, pair number): u, v, the face's
    third vertex o, and per pair the slot (the run of equal (u, v)) it belongs to."""
    F = _faces(F)
    t = np.nonzero(part(F))[0]
    us, vs, os_, hs = [], [], [], []
    for k in range(3):
        for d in range(2):
            us.append(F[t, k])
            vs.append(F[t, (k + 1 + d) % 3])
            os_.append(F[t, (k + 2 - d) % 3])
            hs.append(6 * t + 2 * k + d)
    u, v, o, h = (np.concatenate(x) if len(t) else np.zeros(0, np.int64) for x in (us, vs, os_, hs))
    order = np.lexsort((h, v, u))
    u, v, o = u[order], v[order], o[order]
    head = np.ones(len(u), bool)
    head[1:] = (u[1:] != u[:-1]) | (v[1:] != v[:-1])
    slot = np.cumsum(head) - 1
    return u, v, o, slot, head


def adjacency(V, F):
    """dict: row_off [V + 1], nbr, vflags [V], corner_off [V + 1], corner -- all int64."""
    nv = len(_v32(V))
    F = _faces(F)
    u, v, _, slot, head = _pairs(F)
    faces_on = np.bincount(slot, minlength=int(head.sum()))           # faces on the edge of every slot
    su, nbr = u[head], v[head]
    row_off = np.concatenate([[0], np.cumsum(np.bincount(su, minlength=nv))]).astype(np.int64)
    vflags = (np.diff(row_off) > 0).astype(np.int64)
    vflags |= 2 * (np.bincount(su, weights=faces_on == 1, minlength=nv) > 0)
    vflags |= 4 * (np.bincount(su, weights=faces_on >= 3, minlength=nv) > 0)
    t = np.nonzero(part(F))[0]
    cv = F[t].reshape(-1)
    cc = (3 * t[:, None] + np.arange(3)).reshape(-1)
    order = np.lexsort((cc, cv))
    corner_off = np.concatenate([[0], np.cumsum(np.bincount(cv, minlength=nv))]).astype(np.int64)
    return dict(row_off=row_off, nbr=nbr.astype(np.int64), vflags=vflags.astype(np.int64), corner_off=corner_off,
                corner=cc[order].astype(np.int64), slot_vertex=su, slot_faces=faces_on)


def vertex_normals(V, F, mode=ANGLE):
    """(normals [V, 3] float64 = s / |s| or 0, s [V, 3] the sums, lengths [V] the sums of the terms' lengths)."""
    V32, F = _v32(V), _faces(F)
    P = V32.astype(np.float64)
    adj = adjacency(V32, F)
    c = adj['corner']
    t, k = c // 3, c % 3
    at = np.repeat(np.arange(len(P)), np.diff(adj['corner_off']))      # the vertex of every listed corner
    a, b, cc = P[F[t, 0]], P[F[t, 1]], P[F[t, 2]]
    n = _cross(b - a, cc - a)
    flat = (n == 0).all(axis=1)
    term = n.copy()
    with np.errstate(all='ignore'):
        if mode != AREA:
            scale = np.ones(len(c))
            if mode == ANGLE:
                p = P[F[t, k]]
                u, w = P[F[t, (k + 1) % 3]] - p, P[F[t, (k + 2) % 3]] - p
                scale = np.arctan2(_len(_cross(u, w)), _dot(u, w))
            term = (n / _len(n)[:, None]) * scale[:, None]
    term[flat] = 0.0
    keep = ~flat
    s = np.zeros((len(P), 3))
    np.add.at(s, at[keep], term[keep])                                 # in corner order
    lengths = np.zeros(len(P))
    np.add.at(lengths, at[keep], _len(term[keep]))
    ln = _len(s)
    with np.errstate(all='ignore'):
        normals = np.where((ln > 0)[:, None], s / ln[:, None], 0.0)
    return normals, s, lengths


def smooth(V, F, iterations=10, lam=0.5, mu=-0.53, weights=0, boundary=FIXED, shuffle=None):
    """The fp64 state [V, 3] after ``iterations`` (mu None or 0: plain Laplacian).  A vertex that does not move keeps
    the widened input.  shuffle (a numpy Generator): add every row's terms in a random order instead of the
    contract's -- a measuring device for the tests' tolerance, never the contract."""
    V32, F = _v32(V), _faces(F)
    P = V32.astype(np.float64)
    u, v, o, slot, head = _pairs(F)
    adj = adjacency(V32, F)
    I, J, faces_on, flags = adj['slot_vertex'], adj['nbr'], adj['slot_faces'], adj['vflags']
    wgt = np.ones(len(I))
    if weights:
        a, b = P[u] - P[o], P[v] - P[o]
        ln = _len(_cross(a, b))
        with np.errstate(all='ignore'):
            cot = np.where(ln > 0, _dot(a, b) / ln, 0.0)
        total = np.zeros(len(I))
        np.add.at(total, slot, cot)                                    # pairs of a slot in the order of i's corners
        half = 0.5 * total
        wgt = np.where(half > 0, half, 0.0)
    used, bnd = (flags & 1) > 0, (flags & 2) > 0
    moves = used & ~(bnd & (boundary == FIXED))
    slides = used & bnd & (boundary == SLIDE)
    wgt = np.where(slides[I], (faces_on == 1).astype(np.float64), wgt)
    order = np.arange(len(I))
    if shuffle is not None:
        order = shuffle.permutation(len(I))
    Io, Jo, Wo = I[order], J[order], wgt[order]
    W = np.zeros(len(P))
    np.add.at(W, Io, Wo)
    go = moves & (W > 0)
    steps = [lam] if not mu else [lam, mu]
    for _ in range(int(iterations)):
        for s in steps:
            A = np.zeros((len(P), 3))
            np.add.at(A, Io, Wo[:, None] * (P[Jo] - P[Io]))
            with np.errstate(all='ignore'):
                new = P + s * (A / W[:, None])
            P = np.where(go[:, None], new, P)
    return P
