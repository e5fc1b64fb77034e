"""float64 numpy restatement of what octfusion_amd.reconstruct adds, for the tests.

  * oriented surface sampler (include/ofx.h, ofx_surface_sample_oriented): the draws of tests/metrics_oracle.py plus
    the unit normal (B - A) x (C - A) / |.| of each drawn triangle, from the un-normalised vertices;
  * calc_chamfer (reference utils/util_dualoctree.py:152-168) on given point sets, by brute force: the two directed mean
    squared nearest-neighbour distances x 1e5, in the reference's order (a: from the points of b to a; b: from a to b);
  * the PLY layout mesh.write_ply writes (binary little-endian, float32 x y z [nx ny nz]; points2ply, :171-197).
"""
import numpy as np

import metrics_oracle as MO

CHAMFER_SCALE = 1.0e5


def face_normals(verts, faces):
    """[F, 3] unit normals (zero rows for zero-area faces) and [F] twice the areas, float64 from the fp32 vertices."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    c = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    a2 = np.linalg.norm(c, axis=1)
    return c / np.where(a2 > 0, a2, 1.0)[:, None], a2


def sample_surface_oriented(verts, faces, n, seed=0, shape=0, normalize=True):
    """(points [n, 3], normals [n, 3], triangle [n]) of the oriented sampler contract on one mesh."""
    pts, t = MO.sample_surface(verts, faces, n, seed=seed, shape=shape, normalize=normalize)
    return pts, face_normals(verts, faces)[0][t], t


def min_angles_deg(verts, faces):
    """[F] smallest interior angle of every triangle, degrees."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    out = np.full(len(f), 180.0)
    for k in range(3):
        a, b, c = v[f[:, k]], v[f[:, (k + 1) % 3]], v[f[:, (k + 2) % 3]]
        e0, e1 = b - a, c - a
        cos = (e0 * e1).sum(1) / np.maximum(np.linalg.norm(e0, axis=1) * np.linalg.norm(e1, axis=1), 1e-300)
        out = np.minimum(out, np.degrees(np.arccos(np.clip(cos, -1, 1))))
    return out


def _min_d2(x, y, chunk=1024):
    """[len(x)] squared distance from each point of x to its nearest point of y (brute force, chunked)."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    out = np.empty(len(x))
    for lo in range(0, len(x), chunk):
        d = x[lo:lo + chunk, None, :] - y[None, :, :]
        out[lo:lo + chunk] = (d * d).sum(2).min(1)
    return out


def chamfer(points_a, points_b):
    """calc_chamfer on given samples: (mean_{p in b} min_{q in a} |p - q|^2, mean_{p in a} min_{q in b} |p - q|^2)
    x 1e5 -- kdtree_a.query(points_b) first, as the reference."""
    return (float(_min_d2(points_b, points_a).mean() * CHAMFER_SCALE),
            float(_min_d2(points_a, points_b).mean() * CHAMFER_SCALE))


def chamfer_kdtree(points_a, points_b):
    """The reference's own arithmetic (scipy.spatial.cKDTree), where scipy is installed; None otherwise."""
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return None
    da, _ = cKDTree(np.asarray(points_a, np.float64)).query(np.asarray(points_b, np.float64))
    db, _ = cKDTree(np.asarray(points_b, np.float64)).query(np.asarray(points_a, np.float64))
    return float(np.mean(np.square(da)) * CHAMFER_SCALE), float(np.mean(np.square(db)) * CHAMFER_SCALE)


def cube_lattice(m, lo=0.0, hi=1.0):
    """The (m + 1)^3 - (m - 1)^3 lattice points on the surface of the cube [lo, hi]^3, spacing (hi - lo) / m."""
    g = np.arange(m + 1)
    I, J, K = np.meshgrid(g, g, g, indexing='ij')
    on = (I == 0) | (I == m) | (J == 0) | (J == m) | (K == 0) | (K == m)
    return np.stack([I[on], J[on], K[on]], 1).astype(np.float64) * ((hi - lo) / m) + lo


def ply_bytes(points, normals=None):
    """The file mesh.write_ply must produce, byte for byte."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    names = ['x', 'y', 'z']
    cols = [p]
    if normals is not None:
        cols.append(np.asarray(normals, np.float32).reshape(-1, 3))
        names += ['nx', 'ny', 'nz']
    head = 'ply\nformat binary_little_endian 1.0\nelement vertex %d\n' % len(p)
    head += ''.join('property float %s\n' % k for k in names) + 'end_header\n'
    return head.encode('ascii') + np.concatenate(cols, 1).astype('<f4').tobytes()


# ---- small meshes the CPU and GPU tests share ---------------------------------------------------------------------
def cube_mesh(half=0.5, centre=(0.0, 0.0, 0.0)):
    """Axis-aligned cube, 8 vertices, 12 outward-wound triangles."""
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32) * half
    v = v + np.asarray(centre, np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                  [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    return v, f


def tetrahedron():
    v = np.array([[0.9, 0.1, -0.2], [-0.4, 0.8, 0.1], [-0.5, -0.7, 0.3], [0.1, 0.05, 1.1]], np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)
    return v, f


def height_field(nx=10, ny=15):
    """2 * nx * ny triangles of a bumpy sheet (an open mesh, off-centre and not unit-sized, all angles far from 0)."""
    gx, gy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing='ij')
    z = 0.35 * np.sin(gx * 0.7) * np.cos(gy * 0.5)
    v = np.stack([gx * 0.3 + 2.0, gy * 0.3 - 1.0, z + 0.5], -1).reshape(-1, 3).astype(np.float32)
    idx = lambda i, j: i * (ny + 1) + j                                   # noqa: E731
    f = []
    for i in range(nx):
        for j in range(ny):
            f += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    return v, np.asarray(f, np.int32)
