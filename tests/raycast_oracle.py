"""Float64 oracle of the ray -> mesh contract (include/ofx.h, csrc/ofx_raycast.hip): numpy only, no project imports.

  cast            the contract, brute force over every (ray, triangle) pair: Woop, Benthin and Wald's watertight test in
                  the order of operations include/ofx.h gives.  The kernel's det (Kahan's fma form: the correct sign, an
                  error below 2 ulp) is restated with error-free products (Veltkamp / Dekker), which numpy can do: the
                  signs of U, V, W -- all a hit depends on -- are the exact ones on both sides; the values may differ in
                  the last bits, so tests compare t within a tolerance and faces through the oracle's own t of the
                  RETURNED face ('pair_t').
  moller_trumbore an INDEPENDENT intersection (Moeller and Trumbore 1997, float64, no epsilon): used for values only;
                  it is not watertight and not the contract.
  margin          per ray, the smallest |min(b0, b1, b2)| over all triangles with a non-zero determinant, b the
                  normalised edge functions (barycentric coordinates of the ray in the triangle): how far the ray is
                  from the nearest triangle boundary it could cross, whether it hits or misses.  Rays with a margin
                  below 1e-6 are left out of comparisons between DIFFERENT formulations (hit / miss and the face may
                  legitimately differ there); tests/test_raycast_oracle.py checks that they are at most 1 %.

The mesh makers are ``mesh2sdf_oracle``'s (imported, not copied).
"""
import numpy as np

import mesh2sdf_oracle as O

CHUNK = 1 << 19           # (ray, triangle) pairs evaluated at once
MARGIN = 1e-6
IMAGE_MISMATCH = 8        # image_mismatch(sphere, 32)[0], asserted in tests/test_raycast_oracle.py


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _two_prod(a, b):
    """(p, e) with p = fl(a b) and p + e = a b exactly (Dekker's product on Veltkamp's split; no overflow here)."""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def det2(a, b, c, d):
    """a b - c d with the exact sign: both products error-free, the high parts subtracted first (exact by Sterbenz where
    they are close, dominant where they are not), then the low parts."""
    p, e = _two_prod(a, b)
    q, f = _two_prod(c, d)
    return (p - q) + (e - f)


def _take(A, k):
    return np.take_along_axis(A, k[..., None], axis=-1)[..., 0]


def _ray_frame(Org, Dir):
    ad = np.abs(Dir)
    kz = np.argmax(ad, axis=1)                              # the first of equal maxima: the lowest index
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    neg = _take(Dir, kz) < 0
    kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
    dz = _take(Dir, kz)
    return kx, ky, kz, _take(Dir, kx) / dz, _take(Dir, ky) / dz, 1.0 / dz


def valid(Org, Dir):
    """[n] bool: every component finite and a direction that is not zero."""
    return np.isfinite(Org).all(1) & np.isfinite(Dir).all(1) & (Dir != 0).any(1)


def pairs(Org, Dir, V, F):
    """(hit [n, m] bool, t [n, m], bmin [n, m]) of every (ray, triangle) pair, before the range test: the contract's
    three edge functions, its t = ((U Az + V Bz) + W Cz) / D, and min(U, V, W) / D (NaN where D == 0)."""
    n, m = len(Org), len(F)
    hit = np.zeros((n, m), bool)
    t = np.full((n, m), np.nan)
    bmin = np.full((n, m), np.nan)
    step = max(1, CHUNK // max(m, 1))
    tri = V[F]                                              # [m, 3, 3]
    with np.errstate(all='ignore'):
        for lo in range(0, n, step):
            o, d = Org[lo:lo + step], Dir[lo:lo + step]
            kx, ky, kz, sx, sy, sz = _ray_frame(o, d)
            A = tri[None] - o[:, None, None, :]             # [r, m, 3 corners, 3 axes]
            r = len(o)

            def axis(k):
                idx = np.broadcast_to(k[:, None, None, None], (r, m, 3, 1))
                return np.take_along_axis(A, idx, axis=3)[..., 0]
            az = axis(kz)
            x = axis(kx) - sx[:, None, None] * az
            y = axis(ky) - sy[:, None, None] * az
            z = sz[:, None, None] * az
            U = det2(x[..., 2], y[..., 1], y[..., 2], x[..., 1])
            Vv = det2(x[..., 0], y[..., 2], y[..., 0], x[..., 2])
            W = det2(x[..., 1], y[..., 0], y[..., 1], x[..., 0])
            D = (U + Vv) + W
            same = ((U >= 0) & (Vv >= 0) & (W >= 0)) | ((U <= 0) & (Vv <= 0) & (W <= 0))
            ok = same & (D != 0)
            tt = ((U * z[..., 0] + Vv * z[..., 1]) + W * z[..., 2]) / D
            hit[lo:lo + step] = ok
            t[lo:lo + step] = np.where(D != 0, tt, np.nan)
            bmin[lo:lo + step] = np.where(D != 0, np.minimum(np.minimum(U, Vv), W) / D, np.nan)
    return hit, t, bmin


def _in_range(t, tmin, tmax):
    with np.errstate(all='ignore'):
        tf = t.astype(np.float32)
        return (tf >= np.float32(tmin)) & (tf <= np.float32(tmax)) & np.isfinite(tf)


def cast(Org, Dir, V, F, tmin=0.0, tmax=np.inf):
    """The contract.  dict of t [n] float64 (inf: miss; the device rounds it to fp32), face [n] int64 (-1: miss), margin
    [n], point [n, 3] (org + t dir; NaN for a miss), cos [n] (NaN for a miss), all [n, m] arrays of ``pairs`` under
    'pair_hit' (range test included) and 'pair_t'."""
    Org, Dir = np.asarray(Org, np.float64).reshape(-1, 3), np.asarray(Dir, np.float64).reshape(-1, 3)
    V, F = np.asarray(V, np.float64), np.asarray(F, np.int64).reshape(-1, 3)
    n = len(Org)
    good = valid(Org, Dir)
    o = np.where(good[:, None], Org, 0.0)
    d = np.where(good[:, None], Dir, [0.0, 0.0, 1.0])
    hit, t, bmin = pairs(o, d, V, F)
    hit = hit & _in_range(t, tmin, tmax) & good[:, None]
    tt = np.where(hit, t, np.inf)
    face = np.argmin(tt, axis=1)                            # the lowest index among equal doubles
    best = tt[np.arange(n), face]
    miss = ~np.isfinite(best)
    face = np.where(miss, -1, face)
    with np.errstate(all='ignore'):
        margin = np.nanmin(np.abs(bmin), axis=1) if len(F) else np.full(n, np.inf)
    margin = np.where(np.isnan(margin), np.inf, margin)
    nrm = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    with np.errstate(all='ignore'):
        cs = np.einsum('ik,ik->i', nrm[face], d) / (np.linalg.norm(nrm[face], axis=1) * np.linalg.norm(d, axis=1))
        point = o + best[:, None] * d
    return dict(t=best, face=face, margin=np.where(good, margin, np.inf), point=np.where(miss[:, None], np.nan, point),
                cos=np.where(miss, np.nan, cs), pair_hit=hit, pair_t=t, valid=good)


def moller_trumbore(Org, Dir, V, F, tmin=0.0, tmax=np.inf):
    """(t [n] float64, face [n]): the nearest intersection by Moeller and Trumbore's algorithm, two-sided, inclusive
    borders, no epsilon.  Independent of ``cast``; values only."""
    Org, Dir = np.asarray(Org, np.float64).reshape(-1, 3), np.asarray(Dir, np.float64).reshape(-1, 3)
    V, F = np.asarray(V, np.float64), np.asarray(F, np.int64).reshape(-1, 3)
    n, m = len(Org), len(F)
    a, e1, e2 = V[F[:, 0]][None], (V[F[:, 1]] - V[F[:, 0]])[None], (V[F[:, 2]] - V[F[:, 0]])[None]
    best = np.full(n, np.inf)
    face = np.full(n, -1, np.int64)
    step = max(1, CHUNK // max(m, 1))
    with np.errstate(all='ignore'):
        for lo in range(0, n, step):
            o, d = Org[lo:lo + step, None, :], Dir[lo:lo + step, None, :]
            pv = np.cross(d, e2)
            det = np.einsum('rmk,rmk->rm', np.broadcast_to(e1, pv.shape), pv)
            tv = o - a
            u = np.einsum('rmk,rmk->rm', tv, pv) / det
            qv = np.cross(tv, e1)
            v = np.einsum('rmk,rmk->rm', np.broadcast_to(d, qv.shape), qv) / det
            t = np.einsum('rmk,rmk->rm', np.broadcast_to(e2, qv.shape), qv) / det
            ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= tmin) & (t <= tmax)
            t = np.where(ok, t, np.inf)
            j = np.argmin(t, axis=1)
            best[lo:lo + step] = t[np.arange(len(j)), j]
            face[lo:lo + step] = np.where(np.isfinite(best[lo:lo + step]), j, -1)
    return best, face


# ---------------------------------------------------------------------------------------------------- the test scenes
def shapes():
    """The meshes of the tests: box 12 faces (lattice aligned), icospheres of 320 and 5120 faces, a torus, an open
    plate."""
    return [('box', O.box(-0.5, 0.5)), ('sphere', O.icosphere(2, (0.07, -0.05, 0.03), 0.55)),
            ('sphere4', O.icosphere(4, (0.07, -0.05, 0.03), 0.55)),
            ('torus', O.torus(16, 8, 0.5, 0.2, (0.03, 0.02, -0.04))), ('plate', O.plate())]


CLOSED = ('box', 'sphere', 'torus')
N_RAYS = {'box': 4096, 'sphere': 4096, 'sphere4': 1024, 'torus': 4096, 'plate': 4096}
INTERIOR = {'box': (0.0, 0.0, 0.0), 'sphere': (0.07, -0.05, 0.03), 'torus': (0.53, 0.02, -0.04)}


def ray_set(V, n, seed):
    """(org [n, 3], dir [n, 3]) float64, fp32-representable: half the rays start on the sphere of radius 2 around the
    origin and aim at a point uniform in 1.2 x the mesh's bounding box (about a sixth miss), half start uniform in
    [-1.2, 1.2]^3 (inside and outside the mesh) with a uniform direction; lengths of the directions uniform in
    [0.5, 2]."""
    rng = np.random.default_rng(seed)
    V = np.asarray(V, np.float64)
    lo, hi = V.min(0), V.max(0)
    c, h = (lo + hi) / 2, np.maximum((hi - lo) / 2, 0.05) * 1.2
    k = n // 2
    o1 = rng.normal(size=(k, 3))
    o1 = 2.0 * o1 / np.linalg.norm(o1, axis=1, keepdims=True)
    d1 = c + rng.uniform(-1, 1, (k, 3)) * h - o1
    o2 = rng.uniform(-1.2, 1.2, (n - k, 3))
    d2 = rng.normal(size=(n - k, 3))
    org, dr = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    dr = dr / np.linalg.norm(dr, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))
    return _f32(org), _f32(dr)


def ray_sets():
    """name -> (org, dir): the value ray sets of the GPU tests, one per shape of ``shapes()``."""
    return {name: ray_set(m[0], N_RAYS[name], 7 + k) for k, (name, m) in enumerate(shapes())}


def edges(F):
    e = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0)


def interior_rays(name, V, F, n_hashed=4096, seed=23):
    """(org, dir): from the interior origin of a closed shape towards every vertex, every edge midpoint and
    ``n_hashed`` more directions -- rays through the places where a test that is not watertight leaks."""
    o = np.asarray(INTERIOR[name], np.float64)
    V = np.asarray(V, np.float64)
    e = edges(np.asarray(F, np.int64))
    rng = np.random.default_rng(seed)
    d = np.concatenate([V - o, (V[e[:, 0]] + V[e[:, 1]]) / 2 - o, rng.normal(size=(n_hashed, 3))])
    d = _f32(d)
    return np.broadcast_to(_f32(o), d.shape).copy(), d


# ---------------------------------------------------------------------------------------------------- cameras
def camera_rays(pose, size, yfov=np.pi / 3.0):
    """(org [size^2, 3], dir [size^2, 3]) float64, fp32-representable, in ROW-MAJOR pixel order: the pixel-centre rays
    of the renderer's pinhole camera (-z forward, y up, row 0 the top); dir = R (u, v, -1)."""
    pose = np.asarray(pose, np.float64)
    y, x = np.divmod(np.arange(size * size), size)
    th = np.tan(yfov / 2.0)
    u, v = ((x + 0.5) / size * 2.0 - 1.0) * th, (1.0 - (y + 0.5) / size * 2.0) * th
    R = pose[:3, :3]
    d = (u[:, None] * R[:, 0] + v[:, None] * R[:, 1]) + (-1.0) * R[:, 2][None]
    return _f32(np.broadcast_to(pose[:3, 3], d.shape)), _f32(d)


def unit_frame(V):
    """The mesh scaled to the unit sphere as the renderer does (bounding-box centre, largest distance from it), in
    float64, rounded once to fp32."""
    V = np.asarray(V, np.float64)
    c = (V.min(0) + V.max(0)) * 0.5
    r = np.sqrt(((V - c) ** 2).sum(1).max())
    return _f32((V - c) / (r if r > 0 else 1.0))


def face_images(V, F, size):
    """(ray [20, size, size], raster [20, size, size]) face ids (-1 background) of one mesh, scaled to the unit sphere,
    from the 20 FID views: the contract's on the pixel-centre rays, and the rasteriser oracle's (tests/render_oracle.py,
    screen coordinates snapped to 1/256 pixel)."""
    import render_oracle as RO
    Vn = unit_frame(V)
    c, s = RO.normalization(V)
    ray, ras = [], []
    for eye in RO.fid_views():
        pose = RO.look_at(eye)
        proj = RO.project(V, pose, size, c, s)
        ras.append(RO.split_keys(RO.raster(proj[0], proj[1], F, size)[0])[0])
        ray.append(cast(*camera_rays(pose, size), Vn, F)['face'].reshape(size, size))
    return np.stack(ray), np.stack(ras)


def image_mismatch(V, F, size):
    """(pixels whose face ids differ between the two oracles, pixels covered in one and background in the other)."""
    ray, ras = face_images(V, F, size)
    return int((ray != ras).sum()), int(((ray < 0) != (ras < 0)).sum())
