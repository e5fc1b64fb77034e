"""Float64 oracle of the point -> mesh query contract (include/ofx.h, csrc/ofx_meshquery.hip): numpy only, no project
imports, and on purpose NOT the kernel's algorithm.

  closest point  brute force over every (query, triangle) pair with Ericson's region test (Real-Time Collision
                 Detection, 5.1.5: two vertex regions' dot products decide vertex, edge or face, and the point comes
                 from barycentric weights) -- the kernel clamps three segments and projects on the plane.  A zero-area
                 triangle is the nearest of its three edges, each a clamped segment.
  face           numpy's argmin over the faces: the lowest index among equal float64 distances.  The kernel's distances
                 differ in the last bits, so tests never compare indices with this one; they use ``to_face``.
  sign           ``mesh2sdf_oracle.inside``: the winding number, not a ray.

The mesh makers are ``mesh2sdf_oracle``'s (imported, not copied).
"""
import numpy as np

import mesh2sdf_oracle as O

CHUNK = 1 << 20           # (query, triangle) pairs evaluated at once


def _dot(a, b):
    return np.einsum('...k,...k->...', a, b)


def _safe(x, y):
    return x / np.where(y != 0, y, 1.0)


def _on_segment(p, a, b):
    e = b - a
    ee = _dot(e, e)
    t = np.clip(np.where(ee > 0, _safe(_dot(p - a, e), ee), 0.0), 0.0, 1.0)
    return a + t[..., None] * e


def closest_on_triangles(p, a, b, c):
    """Closest point of the triangles (a, b, c) to the points p; all [..., 3], broadcast together."""
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    den = _safe(1.0, va + vb + vc)
    out = a + ab * (vb * den)[..., None] + ac * (vc * den)[..., None]                    # interior
    regions = [
        ((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), b + (c - b) * _safe(d4 - d3, (d4 - d3) + (d5 - d6))[..., None]),
        ((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + ac * _safe(d2, d2 - d6)[..., None]),
        ((d6 >= 0) & (d5 <= d6), c),
        ((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + ab * _safe(d1, d1 - d3)[..., None]),
        ((d3 >= 0) & (d4 <= d3), b),
        ((d1 <= 0) & (d2 <= 0), a),
    ]
    for cond, val in regions:                                # Ericson's order is the reverse: the last one set wins
        out = np.where(cond[..., None], val, out)
    # zero area: the nearest of the three edges
    n = np.cross(ab, ac)
    flat = _dot(n, n) == 0
    if flat.any():
        cand = np.stack([_on_segment(p, a, b), _on_segment(p, b, c), _on_segment(p, c, a)])
        dd = _dot(p - cand, p - cand)
        best = np.take_along_axis(cand, np.argmin(dd, axis=0)[None, ..., None], axis=0)[0]
        out = np.where(flat[..., None], best, out)
    return out


def query(P, V, F):
    """(d [n], face [n], point [n, 3]) float64 / int64: distance from every point of P to the mesh (V, F), the lowest
    face that attains it, and the closest point on that face."""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    V = np.asarray(V, np.float64)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    a, b, c = V[F[:, 0]][None], V[F[:, 1]][None], V[F[:, 2]][None]
    d = np.empty(len(P))
    face = np.empty(len(P), np.int64)
    point = np.empty((len(P), 3))
    step = max(1, CHUNK // max(len(F), 1))
    for lo in range(0, len(P), step):
        p = P[lo:lo + step, None, :]
        cl = closest_on_triangles(p, a, b, c)
        d2 = _dot(p - cl, p - cl)
        j = np.argmin(d2, axis=1)
        rows = np.arange(len(j))
        d[lo:lo + step] = np.sqrt(d2[rows, j])
        face[lo:lo + step] = j
        point[lo:lo + step] = cl[rows, j]
    return d, face, point


def to_face(P, V, F, face):
    """(d [n], point [n, 3]): distance from point i of P to triangle face[i] alone, and the closest point on it."""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    V = np.asarray(V, np.float64)
    t = np.asarray(F, np.int64).reshape(-1, 3)[np.asarray(face, np.int64)]
    cl = closest_on_triangles(P, V[t[:, 0]], V[t[:, 1]], V[t[:, 2]])
    return np.sqrt(_dot(P - cl, P - cl)), cl


def inside(P, V, F):
    """[n] bool: the parity sign, from the winding number (mesh2sdf_oracle.inside)."""
    return O.inside(P, V, F)


def all_faces(P, V, F):
    """[n, m] float64: the distance from every point of P to every triangle of the mesh alone."""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    V = np.asarray(V, np.float64)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    out = np.empty((len(P), len(F)))
    step = max(1, CHUNK // max(len(F), 1))
    for lo in range(0, len(P), step):
        p = P[lo:lo + step, None, :]
        cl = closest_on_triangles(p, V[F[:, 0]][None], V[F[:, 1]][None], V[F[:, 2]][None])
        out[lo:lo + step] = np.sqrt(_dot(p - cl, p - cl))
    return out


def shapes():
    """The four meshes of the tests, in the order their query sets are drawn."""
    return [('sphere', O.icosphere(2, (0.07, -0.05, 0.03), 0.55)),
            ('torus', O.torus(16, 8, 0.5, 0.2, (0.03, 0.02, -0.04))), ('box', O.box()), ('plate', O.plate())]


def query_sets(meshes, seed=7, n_uniform=3072, n_near=1024):
    """One [n_uniform + n_near, 3] float64 (fp32-representable) query set per mesh of `meshes`, drawn in turn from ONE
    default_rng(seed): n_uniform points uniform in [-1.2, 1.2]^3, then n_near mesh vertices (rng.integers, with
    replacement) jittered by N(0, 0.02)."""
    rng = np.random.default_rng(seed)
    out = []
    for m in meshes:
        V = np.asarray(m[0], np.float64)
        u = rng.uniform(-1.2, 1.2, (n_uniform, 3))
        pick = rng.integers(0, len(V), n_near)
        near = V[pick] + rng.normal(0.0, 0.02, (n_near, 3))
        out.append(np.concatenate([u, near]).astype(np.float32).astype(np.float64))
    return out
