"""Numpy restatement of the voxel-mesh contract (include/ofx.h, 'voxel meshes of octrees'; the reference's _voxel2mesh,
models/networks/diffusion_networks/ldm_diffusion_util.py:353-446), vectorised: shifted copies of a zero-padded
occupancy grid instead of a loop over the occupied voxels.  tests/golden/g_voxmesh.pt pins it to the reference's own
output; the GPU tests use it at the sizes the golden file does not hold.

Cell (x, y, z) is occupied iff its value is finite and > threshold.  A face is exposed iff the neighbour is not
occupied (outside the grid: never occupied).  Quads ascend in (x, y, z, face) with the faces +z, -z, -x, +x, +y, -y;
QUAD holds each face's four corner offsets, TRI its two triangles as indices into those four.
"""
import numpy as np

DIRS = np.array([[0, 0, 1], [0, 0, -1], [-1, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0]])
QUAD = np.array([[[0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]],
                 [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]],
                 [[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1]],
                 [[1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]],
                 [[0, 1, 0], [1, 1, 0], [0, 1, 1], [1, 1, 1]],
                 [[0, 0, 0], [1, 0, 0], [0, 0, 1], [1, 0, 1]]])
TRI = np.array([[[0, 1, 3], [1, 2, 3]], [[1, 0, 3], [2, 1, 3]], [[0, 1, 3], [2, 0, 3]],
                [[1, 0, 3], [0, 2, 3]], [[1, 0, 3], [0, 2, 3]], [[0, 1, 3], [2, 0, 3]]])


def occupancy(grid, threshold=0.4):
    grid = np.asarray(grid)
    with np.errstate(invalid='ignore'):
        return np.isfinite(grid) & (grid > threshold)


def quads(occ):
    """(cells [Q, 3], face ids [Q]) of the exposed faces of a boolean grid, in emission order."""
    R = occ.shape[0]
    pad = np.zeros((R + 2,) * 3, bool)
    pad[1:-1, 1:-1, 1:-1] = occ
    exposed = np.stack([occ & ~pad[1 + dx:R + 1 + dx, 1 + dy:R + 1 + dy, 1 + dz:R + 1 + dz] for dx, dy, dz in DIRS],
                       axis=-1)
    x, y, z, k = np.nonzero(exposed)
    return np.stack([x, y, z], 1), k


def corners(occ):
    """Integer lattice corners [Q, 4, 3] of the quads."""
    cells, k = quads(occ)
    return cells[:, None, :] + QUAD[k]


def _coords(c, R):
    return (c * (2.0 / R) - 1.0).astype(np.float32)           # exact: R is a power of two


def unwelded(grid, threshold=0.4):
    """(verts [4Q, 3] float32, faces [2Q, 3] int32): four vertices per quad, the reference's arrays."""
    occ = occupancy(grid, threshold)
    R = occ.shape[0]
    cells, k = quads(occ)
    c = cells[:, None, :] + QUAD[k]
    faces = TRI[k] + 4 * np.arange(len(k))[:, None, None]
    return _coords(c.reshape(-1, 3), R), faces.reshape(-1, 3).astype(np.int32)


def corner_index(c, R):
    return (c[..., 0] * (R + 1) + c[..., 1]) * (R + 1) + c[..., 2]


def weld(verts, faces, R):
    """The welding rule on unwelded arrays: every used lattice corner once, in ascending corner index."""
    c = np.rint((verts.astype(np.float64) + 1.0) * (R / 2.0)).astype(np.int64)
    idx = corner_index(c, R)
    uniq, inv = np.unique(idx, return_inverse=True)
    r1 = R + 1
    cw = np.stack([uniq // (r1 * r1), (uniq // r1) % r1, uniq % r1], 1)
    return _coords(cw, R).reshape(-1, 3), inv.reshape(-1)[faces].astype(np.int32).reshape(-1, 3)


def welded(grid, threshold=0.4):
    v, f = unwelded(grid, threshold)
    return weld(v, f, np.asarray(grid).shape[0])


def mesh(grid, threshold=0.4, weld=True):
    return welded(grid, threshold) if weld else unwelded(grid, threshold)


# ---- seeded grids of the tests --------------------------------------------------------------------------------------
def random_grid(R, fill=0.5, seed=0):
    return (np.random.default_rng(seed).random((R, R, R)) < fill).astype(np.float32)


def checkerboard(R):
    g = np.indices((R, R, R)).sum(0) % 2
    return g.astype(np.float32)


def directed_edge_balance(faces):
    """Every directed edge occurs as often as its reverse: closed and consistently oriented."""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    n = int(e.max()) + 1
    fwd = np.sort(e[:, 0] * n + e[:, 1])
    rev = np.sort(e[:, 1] * n + e[:, 0])
    return np.array_equal(fwd, rev)


def signed_volume(verts, faces):
    v = verts.astype(np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0)
