"""Float64 oracle of the mesh -> SDF lattice contract (include/ofx.h, csrc/ofx_mesh2sdf.hip): numpy only, no project
imports, and on purpose NOT the kernel's algorithm.

  magnitude  brute force over every (point, triangle) pair: closest point on the triangle by Ericson's region test
             (Real-Time Collision Detection, 5.1.5); a zero-area triangle is the nearest of its three edges, each a
             clamped segment (a zero-length edge is its end point);
  sign       the winding number from van Oosterom & Strackee's solid-angle formula, not a ray: inside iff
             round(winding) is odd.  For a closed, consistently oriented surface that is the parity of the crossings
             of any ray, so it agrees with the kernel's rule wherever the point is off the surface.

Mesh makers round their vertices through fp32, so the oracle and the device see the same coordinates.
"""
import numpy as np

CHUNK = 1 << 21           # (point, triangle) pairs evaluated at once


def _f32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def lattice(S):
    """[S^3, 3] float64 lattice points p = 2 i / S - 1, x slowest."""
    ax = 2 * np.arange(S) / S - 1
    return np.stack(np.meshgrid(ax, ax, ax, indexing='ij'), axis=-1).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------- mesh makers
def icosphere(sub=2, centre=(0.0, 0.0, 0.0), r=1.0):
    """(verts [V, 3] float64 (fp32-representable), faces [20 * 4^sub, 3] int32), outward."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(sub):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return _f32(np.asarray(v) * r + np.asarray(centre, np.float64)), np.asarray(f, np.int32)


def torus(nu=16, nv=8, R=0.5, r=0.2, centre=(0.0, 0.0, 0.0)):
    """A torus around the z axis: nu segments around the axis, nv around the tube; 2 nu nv faces, outward."""
    u = 2 * np.pi * np.arange(nu) / nu
    w = 2 * np.pi * np.arange(nv) / nv
    uu, ww = np.meshgrid(u, w, indexing='ij')
    v = np.stack([(R + r * np.cos(ww)) * np.cos(uu), (R + r * np.cos(ww)) * np.sin(uu), r * np.sin(ww)], -1)
    f = []
    for i in range(nu):
        for j in range(nv):
            a, b = i * nv + j, ((i + 1) % nu) * nv + j
            c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            f += [(a, b, c), (a, c, d)]
    return _f32(v.reshape(-1, 3) + np.asarray(centre, np.float64)), np.asarray(f, np.int32)


def box(lo=-0.5, hi=0.5):
    """An axis-aligned box of 12 outward triangles; lo / hi: scalars or 3-vectors."""
    lo = np.broadcast_to(np.asarray(lo, np.float64), (3,))
    hi = np.broadcast_to(np.asarray(hi, np.float64), (3,))
    v = np.asarray([[(hi if (i >> (2 - a)) & 1 else lo)[a] for a in range(3)] for i in range(8)])   # index = x y z bits
    f = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
         (1, 5, 7), (1, 7, 3)]
    return _f32(v), np.asarray(f, np.int32)


def plate(half=0.5, x=0.03):
    """An open square of 2 triangles in the plane x = const: not watertight."""
    v = np.asarray([(x, -half, -half), (x, half, -half), (x, half, half), (x, -half, half)])
    return _f32(v), np.asarray([(0, 1, 2), (0, 2, 3)], np.int32)


def merge(*meshes):
    """One mesh holding all of `meshes`."""
    vs, fs, n = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(np.asarray(f, np.int64) + n)
        n += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


# ---------------------------------------------------------------------------------------------------- distance
def _dot(a, b):
    return np.einsum('...k,...k->...', a, b)


def _segment2(p, a, b):
    e = b - a
    ee = _dot(e, e)
    t = np.where(ee > 0, _dot(p - a, e) / np.where(ee > 0, ee, 1.0), 0.0)
    d = p - (a + np.clip(t, 0.0, 1.0)[..., None] * e)
    return _dot(d, d)


def _closest2(p, a, b, c):
    """Squared distance from p [n, 1, 3] to the triangles a, b, c [1, m, 3]: Ericson's region test."""
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    va = d3 * d6 - d5 * d4
    vb = d5 * d2 - d1 * d6
    vc = d1 * d4 - d3 * d2

    def div(x, y):
        return x / np.where(y != 0, y, 1.0)
    shape = np.broadcast(d1, d2).shape
    a, ab, ac = (np.broadcast_to(t, shape + (3,)) for t in (a, ab, ac))
    den = div(1.0, va + vb + vc)
    q = a + ab * (vb * den)[..., None] + ac * (vc * den)[..., None]                       # the face
    conds = [
        ((d1 <= 0) & (d2 <= 0), a),
        ((d3 >= 0) & (d4 <= d3), a + ab),
        ((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + ab * div(d1, d1 - d3)[..., None]),
        ((d6 >= 0) & (d5 <= d6), a + ac),
        ((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + ac * div(d2, d2 - d6)[..., None]),
        ((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0),
         a + ab + (ac - ab) * div(d4 - d3, (d4 - d3) + (d5 - d6))[..., None]),
    ]
    for cond, val in reversed(conds):                       # the first true condition wins
        q = np.where(cond[..., None], val, q)
    d = np.broadcast_to(p, shape + (3,)) - q
    return _dot(d, d)


def udf(P, V, F):
    """[n] float64 distance from every point of P [n, 3] to the mesh (V, F)."""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    V = np.asarray(V, np.float64)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    n = np.cross(b - a, c - a)
    flat = _dot(n, n) == 0                                  # zero area: the nearest of the three edges
    out = np.full(len(P), np.inf)
    step = max(1, CHUNK // max(len(F), 1))
    for lo in range(0, len(P), step):
        p = P[lo:lo + step, None, :]
        best = np.full(p.shape[0], np.inf)
        if (~flat).any():
            best = _closest2(p, a[None, ~flat], b[None, ~flat], c[None, ~flat]).min(axis=1)
        if flat.any():
            fa, fb, fc = a[None, flat], b[None, flat], c[None, flat]
            seg = np.minimum(np.minimum(_segment2(p, fa, fb), _segment2(p, fb, fc)), _segment2(p, fc, fa))
            best = np.minimum(best, seg.min(axis=1))
        out[lo:lo + step] = best
    return np.sqrt(out)


# ---------------------------------------------------------------------------------------------------- sign
def winding(P, V, F):
    """[n] float64 winding number of the mesh around every point (van Oosterom & Strackee 1983)."""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    V = np.asarray(V, np.float64)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    out = np.empty(len(P))
    step = max(1, CHUNK // max(len(F), 1))
    for lo in range(0, len(P), step):
        p = P[lo:lo + step, None, :]
        a, b, c = V[F[:, 0]][None] - p, V[F[:, 1]][None] - p, V[F[:, 2]][None] - p
        la, lb, lc = (np.sqrt(_dot(t, t)) for t in (a, b, c))
        num = _dot(a, np.cross(b, c))
        den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
        out[lo:lo + step] = (2.0 * np.arctan2(num, den)).sum(axis=1) / (4.0 * np.pi)
    return out


def inside(P, V, F):
    """[n] bool: round(winding) is odd."""
    return np.mod(np.rint(winding(P, V, F)).astype(np.int64), 2) == 1


def sdf(P, V, F):
    """(sdf [n], udf [n]): -udf where round(winding) is odd."""
    d = udf(P, V, F)
    return np.where(inside(P, V, F), -d, d), d
