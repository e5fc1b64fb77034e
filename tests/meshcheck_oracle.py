"""Float64 oracle of the mesh checker's contract (include/ofx.h, csrc/ofx_meshcheck.hip): numpy only, no project
imports, and on purpose NOT the kernels' algorithm -- ``np.unique`` where the device sorts, all pairs where it bins.

  weld       vertices with three equal fp32 coordinates (-0 == +0; a vertex with a non-finite coordinate is alone),
             the representative the lowest index.
  topology   edge, face and vertex counts, ``edge_faces``, components, area and volume of include/ofx.h.
  selfx      per face the number of other faces it intersects and the lowest of them, by the pair rule of the header:
             every i < j whose closed fp32 boxes overlap goes through the predicate.

Arithmetic.  Every 3-D expression is the header's own, operation by operation (numpy rounds every float64 operation
on its own).  The 2-D orientation is the SIGN of a 2 x 2 determinant of rounded differences; the device takes it from
Kahan's fma form, whose relative error is below 1 (Jeannerod, Louvet and Muller 2013), so its sign is the exact one;
here the exact sign comes from a plain evaluation where that is beyond its error bound and from rationals otherwise.
"""
from fractions import Fraction

import numpy as np

K_COUNTS = ['index_degenerate_faces', 'edges', 'boundary_edges', 'nonmanifold_edges', 'inconsistent_edges',
            'duplicate_faces', 'zero_area_faces', 'unreferenced_vertices', 'components']


def _v32(V):
    return np.ascontiguousarray(np.asarray(V, np.float32).reshape(-1, 3))


def _faces(F):
    return np.asarray(F, np.int64).reshape(-1, 3)


# ---- weld ----------------------------------------------------------------------------------------------------------
def weld(V, F):
    """(rep [V], verts [n, 3] fp32, faces [F, 3], index [V]): rep = the lowest index with the same coordinates."""
    V = _v32(V)
    F = _faces(F)
    bits = V.view(np.uint32).astype(np.int64)
    bits[bits == 0x80000000] = 0
    alone = ~np.isfinite(V).all(axis=1)
    rows = np.concatenate([bits, np.where(alone, np.arange(len(V)) + 1, 0)[:, None]], axis=1)
    _, first, inv = np.unique(rows, axis=0, return_index=True, return_inverse=True)
    rep = first[inv.reshape(-1)]
    reps = np.sort(first)
    index = np.searchsorted(reps, rep)
    return rep, V[reps], index[F] if len(F) else F, index


# ---- topology ------------------------------------------------------------------------------------------------------
def _cross(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                     u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)


def _dot(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def index_degenerate(F):
    F = _faces(F)
    return (F[:, 0] == F[:, 1]) | (F[:, 1] == F[:, 2]) | (F[:, 0] == F[:, 2])


def _corners(V, F):
    V = _v32(V).astype(np.float64)
    return V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]


def components(nv, F):
    """Number of connected components that hold a face: two vertices are connected when a face uses both."""
    F = _faces(F)
    lab = np.arange(nv)
    while True:
        m = lab[F].min(axis=1)
        new = lab.copy()
        for k in range(3):
            np.minimum.at(new, F[:, k], m)
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    return len(np.unique(lab[F[:, 0]]))


def topology(V, F):
    """dict: the K_COUNTS, ``edge_faces`` [F, 3], ``area``, ``volume`` and the sums of the absolute terms."""
    V32 = _v32(V)
    F = _faces(F)
    nv, nf = len(V32), len(F)
    deg = index_degenerate(F)
    ok = ~deg
    G = F[ok]
    out = {}
    ef = np.zeros((nf, 3), np.int64)
    if len(G):
        u = G
        v = G[:, [1, 2, 0]]
        lo, hi = np.minimum(u, v), np.maximum(u, v)
        key = (lo * nv + hi).reshape(-1)
        rev = (u > v).reshape(-1).astype(np.int64)
        _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        nrev = np.bincount(inv, weights=rev, minlength=len(cnt)).astype(np.int64)
        bad = (cnt == 2) & (nrev != 1)
        n = cnt[inv]
        ef[ok] = np.where(bad[inv], -n, n).reshape(-1, 3)
        out.update(edges=len(cnt), boundary_edges=int((cnt == 1).sum()), nonmanifold_edges=int((cnt >= 3).sum()),
                   inconsistent_edges=int(bad.sum()))
        out['duplicate_faces'] = len(G) - len(np.unique(np.sort(G, axis=1), axis=0))
        out['unreferenced_vertices'] = nv - len(np.unique(G))
    else:
        out.update(edges=0, boundary_edges=0, nonmanifold_edges=0, inconsistent_edges=0, duplicate_faces=0,
                   unreferenced_vertices=nv)
    a, b, c = _corners(V32, F)
    n = _cross(b - a, c - a)
    out['index_degenerate_faces'] = int(deg.sum())
    out['zero_area_faces'] = int((ok & (n == 0).all(axis=1)).sum())
    out['components'] = components(nv, F)
    ta = np.where(ok, 0.5 * np.sqrt(_dot(n, n)), 0.0)
    tv = np.where(ok, _dot(a, _cross(b, c)) / 6.0, 0.0)
    out.update(edge_faces=ef, area=float(ta.sum()), volume=float(tv.sum()), area_abs=float(np.abs(ta).sum()),
               volume_abs=float(np.abs(tv).sum()))
    return out


def derived(t, nf, nv, pairs=None):
    """The fields mesh_check.check derives from the counts."""
    faces = nf - t['index_degenerate_faces']
    euler = (nv - t['unreferenced_vertices']) - t['edges'] + faces
    closed = t['boundary_edges'] == 0 and faces > 0
    manifold = t['nonmanifold_edges'] == 0
    oriented = t['inconsistent_edges'] == 0
    water = closed and manifold and t['index_degenerate_faces'] == 0 and t['duplicate_faces'] == 0
    genus = (2 * t['components'] - euler) // 2 if water and oriented else None
    return dict(euler=euler, closed=closed, edge_manifold=manifold, oriented=oriented, watertight=water, genus=genus)


# ---- self-intersections --------------------------------------------------------------------------------------------
def _det2_sign(a, b, c, d):
    """Exact sign of a b - c d."""
    x, y = a * b, c * d
    r = x - y
    s = np.sign(r)
    unsure = np.abs(r) <= 8.0 * 2.0 ** -53 * (np.abs(x) + np.abs(y))
    for i in np.nonzero(unsure)[0]:
        e = Fraction(float(a[i])) * Fraction(float(b[i])) - Fraction(float(c[i])) * Fraction(float(d[i]))
        s[i] = (e > 0) - (e < 0)
    return s.astype(np.int64)


def _o2(p, q, r):
    """Orientation of the 2-D points p, q, r [n, 2]: the sign of (q - p) x (r - p) on rounded differences."""
    return _det2_sign(q[:, 0] - p[:, 0], r[:, 1] - p[:, 1], q[:, 1] - p[:, 1], r[:, 0] - p[:, 0])


def _project(n, *pts):
    """The points [m, 3] dropped along the dominant axis of n (ties to the lowest index): axes k + 1, k + 2."""
    k = np.argmax(np.abs(n), axis=1)
    r = np.arange(len(n))
    u, v = (k + 1) % 3, (k + 2) % 3
    return [np.stack([p[r, u], p[r, v]], axis=1) for p in pts]


def _all_one_side(s1, s2, s3):
    return ((s1 >= 0) & (s2 >= 0) & (s3 >= 0)) | ((s1 <= 0) & (s2 <= 0) & (s3 <= 0))


def _seg_cross(p, q, r, s):
    d1, d2, d3, d4 = _o2(p, q, r), _o2(p, q, s), _o2(r, s, p), _o2(r, s, q)
    line = (d1 == 0) & (d2 == 0) & (d3 == 0) & (d4 == 0)
    ax = np.where(np.abs(q[:, 0] - p[:, 0]) >= np.abs(q[:, 1] - p[:, 1]), 0, 1)
    i = np.arange(len(p))
    P, Q, R, S = p[i, ax], q[i, ax], r[i, ax], s[i, ax]
    over = np.maximum(np.minimum(P, Q), np.minimum(R, S)) <= np.minimum(np.maximum(P, Q), np.maximum(R, S))
    return np.where(line, over, (d1 * d2 <= 0) & (d3 * d4 <= 0))


def edge_meets(p, q, a, b, c):
    """[m] bool: the edge p q meets the closed triangle a b c (all [m, 3] float64)."""
    n = _cross(b - a, c - a)
    sp, sq = np.sign(_dot(n, p - a)), np.sign(_dot(n, q - a))
    miss = (sp == sq) & (sp != 0)
    flat = (sp == 0) & (sq == 0)
    d, A, B, C = q - p, a - p, b - p, c - p
    hit = _all_one_side(np.sign(_dot(d, _cross(A, B))), np.sign(_dot(d, _cross(B, C))), np.sign(_dot(d, _cross(C, A))))
    hit = hit & ~miss
    idx = np.nonzero(flat)[0]
    if len(idx):
        P, Q, A2, B2, C2 = _project(n[idx], p[idx], q[idx], a[idx], b[idx], c[idx])
        inside = lambda x: _all_one_side(_o2(A2, B2, x), _o2(B2, C2, x), _o2(C2, A2, x))
        h = inside(P) | inside(Q) | _seg_cross(P, Q, A2, B2) | _seg_cross(P, Q, B2, C2) | _seg_cross(P, Q, C2, A2)
        hit[idx] = h
    return hit


def _fold(Ti, apex, b):
    """k = 2: Ti [m, 3, 3] the lower face, apex [m] the position of its unshared vertex, b [m, 3] the other apex."""
    r = np.arange(len(Ti))
    a, u, v = Ti[r, apex], Ti[r, (apex + 1) % 3], Ti[r, (apex + 2) % 3]
    n = _cross(Ti[:, 1] - Ti[:, 0], Ti[:, 2] - Ti[:, 0])
    flat = _dot(n, b - Ti[:, 0]) == 0
    U, W, A, B = _project(n, u, v, a, b)
    sa, sb = _o2(U, W, A), _o2(U, W, B)
    return flat & (sa != 0) & (sa == sb)


def selfx(V, F):
    """(partners [F], first [F], pairs): the pair rule of include/ofx.h over all i < j."""
    V32 = _v32(V)
    F = _faces(F)
    nf = len(F)
    V64 = V32.astype(np.float64)
    T = V64[F]                                             # [F, 3, 3]
    n = _cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    live = ~index_degenerate(F) & (n != 0).any(axis=1)
    lo, hi = V32[F].min(axis=1), V32[F].max(axis=1)
    I, J = [], []
    for i in np.nonzero(live)[0]:
        j = np.arange(i + 1, nf)
        m = live[j] & (lo[j] <= hi[i]).all(axis=1) & (hi[j] >= lo[i]).all(axis=1)
        j = j[m]
        I.append(np.full(len(j), i))
        J.append(j)
    I = np.concatenate(I) if I else np.zeros(0, np.int64)
    J = np.concatenate(J) if J else np.zeros(0, np.int64)
    same = F[I][:, :, None] == F[J][:, None, :]           # [m, 3 of i, 3 of j]
    si, sj = same.any(axis=2), same.any(axis=1)            # which corners of i / of j are shared
    k = si.sum(axis=1)
    hit = np.zeros(len(I), bool)
    nxt = lambda x: (x + 1) % 3
    # k = 0: any edge of one meets the other
    m = np.nonzero(k == 0)[0]
    for A, B in ((I, J), (J, I)):
        for e in range(3):
            hit[m] |= edge_meets(T[A[m], e], T[A[m], nxt(e)], T[B[m], 0], T[B[m], 1], T[B[m], 2])
    # k = 1: the edges opposite the shared vertex
    m = np.nonzero(k == 1)[0]
    if len(m):
        pi, pj = np.argmax(si[m], axis=1), np.argmax(sj[m], axis=1)
        for A, B, pa in ((I[m], J[m], pi), (J[m], I[m], pj)):
            hit[m] |= edge_meets(T[A, nxt(pa)], T[A, nxt(nxt(pa))], T[B, 0], T[B, 1], T[B, 2])
    # k = 2: folded flat onto the neighbour
    m = np.nonzero(k == 2)[0]
    if len(m):
        ai, aj = np.argmin(si[m], axis=1), np.argmin(sj[m], axis=1)
        hit[m] = _fold(T[I[m]], ai, T[J[m], aj])
    I, J = I[hit], J[hit]
    partners = np.bincount(I, minlength=nf) + np.bincount(J, minlength=nf)
    first = np.full(nf, nf, np.int64)
    np.minimum.at(first, I, J)
    np.minimum.at(first, J, I)
    first[first == nf] = -1
    return partners.astype(np.int64), first, len(I)
