"""numpy restatement of the marching-cubes contract of csrc/ofx_mesh.hip (octfusion_amd.mesh.marching_cubes).

  * cell (i, j, k), 0 <= i, j, k < R-1; a corner is inside iff v < level; the lattice boundary is not padded;
  * one vertex per lattice edge with exactly one inside endpoint, owned by its lower endpoint a, running +x / +y / +z
    to b; index-space position a + t (b - a), t = (level - v_a) / (v_b - v_a) in fp32 (a difference that overflows
    to +-inf gives t = +-0: the vertex is the owner point); output (p * step + bbmin) *
    scale with step = (bbmax - bbmin) / R; vertex order: owner's linear index (x slowest), then axis x, y, z;
  * triangles from the table of tools/gen_mc_table.py, ordered by cell linear index, then table order; int32,
    0-based into the shape's own vertices.
"""
import os
import sys

import numpy as np

_TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
if _TOOLS not in sys.path:
    sys.path.insert(0, _TOOLS)
import gen_mc_table  # noqa: E402


def tables():
    """(tri [256, 16] int8, -1 padded; ntri [256] uint8) -- the layout ofx_mc_table_host fills."""
    tab = gen_mc_table.table()
    tri = np.full((256, 16), -1, np.int8)
    ntri = np.zeros(256, np.uint8)
    for c, ts in enumerate(tab):
        flat = [e for t in ts for e in t]
        tri[c, :len(flat)] = flat
        ntri[c] = len(ts)
    return tri, ntri


_TRI, _NTRI = tables()
# edge e -> (owner offset dx, dy, dz, axis)
_EDGE = np.array([list(gen_mc_table.edge_owner(e)[0]) + [gen_mc_table.edge_owner(e)[1]] for e in range(12)], np.int64)


def cube_index(inside):
    R = inside.shape[0]
    ci = np.zeros((R - 1,) * 3, np.int64)
    for c in range(8):
        dx, dy, dz = (c >> 2) & 1, (c >> 1) & 1, c & 1
        ci |= inside[dx:R - 1 + dx, dy:R - 1 + dy, dz:R - 1 + dz].astype(np.int64) << c
    return ci


def nonfinite_cells(sdf):
    bad = ~np.isfinite(np.asarray(sdf, np.float32))
    R = bad.shape[0]
    acc = np.zeros((R - 1,) * 3, bool)
    for c in range(8):
        dx, dy, dz = (c >> 2) & 1, (c >> 1) & 1, c & 1
        acc |= bad[dx:R - 1 + dx, dy:R - 1 + dy, dz:R - 1 + dz]
    return int(acc.sum())


def marching_cubes(sdf, level=0.0, bbmin=-0.9, bbmax=0.9, scale=1.0):
    """(verts [V, 3] float32, faces [F, 3] int32) of one lattice [R, R, R]."""
    v = np.ascontiguousarray(np.asarray(sdf, np.float32))
    R = v.shape[0]
    assert v.shape == (R, R, R) and R >= 2
    lev = np.float32(level)
    inside = v < lev
    cr = np.zeros((R, R, R, 3), bool)
    cr[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cr[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cr[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    flat = cr.reshape(-1)
    vid = np.cumsum(flat, dtype=np.int64) - 1
    idx = np.nonzero(flat)[0]
    p, a = idx // 3, idx % 3
    stride = np.array([R * R, R, 1], np.int64)
    vf = v.reshape(-1)
    va, vb = vf[p], vf[p + stride[a]]
    assert va.dtype == vb.dtype == np.float32 and lev.dtype == np.float32      # every operation below rounds to fp32
    with np.errstate(over='ignore'):
        t = ((lev - va) / (vb - va)).astype(np.float32)
    pos = np.stack([p // (R * R), (p // R) % R, p % R], 1).astype(np.float32)
    pos[np.arange(len(p)), a] += t
    step = np.float32((bbmax - bbmin) / R)
    verts = ((pos * step + np.float32(bbmin)) * np.float32(scale)).astype(np.float32)

    ci = cube_index(inside).reshape(-1)
    nt = _NTRI[ci]
    cells = np.nonzero(nt)[0]
    if len(cells) == 0:
        return verts.reshape(-1, 3), np.zeros((0, 3), np.int32)
    c = ci[cells]
    i, j, k = cells // ((R - 1) ** 2), (cells // (R - 1)) % (R - 1), cells % (R - 1)
    rows = _TRI[c][:, :15].reshape(-1, 5, 3).astype(np.int64)
    keep = np.arange(5)[None, :] < nt[cells][:, None].astype(np.int64)
    cell_of = np.repeat(np.arange(len(cells)), 5).reshape(-1, 5)[keep]
    e = rows[keep]                                              # [F, 3] edge ids, cell-major then table order
    own = _EDGE[e]                                              # [F, 3, 4]
    q = ((i[cell_of][:, None] + own[..., 0]) * R + (j[cell_of][:, None] + own[..., 1])) * R + \
        (k[cell_of][:, None] + own[..., 2])
    faces = vid[q * 3 + own[..., 3]]
    assert (faces >= 0).all() and flat[q * 3 + own[..., 3]].all()
    return verts.reshape(-1, 3), faces.astype(np.int32)


# ---- geometry helpers the tests use ------------------------------------------------------------------------------
def directed_edge_balance(faces):
    """True iff every directed edge (a, b) occurs as often as (b, a)."""
    f = np.asarray(faces, np.int64)
    if len(f) == 0:
        return True
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(e.max()) + 1
    fwd = np.sort(e[:, 0] * n + e[:, 1])
    bwd = np.sort(e[:, 1] * n + e[:, 0])
    return bool(np.array_equal(fwd, bwd))


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0)


def area(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    return float(0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1).sum())


def euler(verts, faces):
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = np.unique(np.sort(e, 1), axis=0)
    used = np.unique(f)
    return len(used) - len(e) + len(f)


# ---- fields ------------------------------------------------------------------------------------------------------
def lattice_coords(R, bbmin=-0.9, bbmax=0.9):
    g = (np.arange(R, dtype=np.float32) * np.float32((bbmax - bbmin) / R) + np.float32(bbmin))
    return np.meshgrid(g, g, g, indexing='ij')


def sphere(R, r=0.5, center=(0.013, -0.021, 0.007)):
    x, y, z = lattice_coords(R)
    return (np.sqrt((x - center[0]) ** 2 + (y - center[1]) ** 2 + (z - center[2]) ** 2) - r).astype(np.float32)


def torus(R, rmaj=0.5, rmin=0.2):
    x, y, z = lattice_coords(R)
    q = np.sqrt(x ** 2 + y ** 2) - rmaj
    return (np.sqrt(q ** 2 + z ** 2) - rmin).astype(np.float32)


def gaussians(R, n=6, seed=0):
    rng = np.random.default_rng(seed)
    x, y, z = lattice_coords(R)
    f = np.full(x.shape, 0.35, np.float32)
    for _ in range(n):
        c = rng.uniform(-0.5, 0.5, 3)
        s = rng.uniform(0.1, 0.3)
        f -= np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / (2 * s * s)).astype(np.float32)
    return f.astype(np.float32)


def random_signs(R, seed=0, border=True):
    """Random +-1 field; border=True keeps the lattice boundary outside (+1) so the surface is closed."""
    rng = np.random.default_rng(seed)
    f = np.where(rng.random((R, R, R)) < 0.5, -1.0, 1.0).astype(np.float32)
    if border:
        f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = 1, 1, 1, 1, 1, 1
    return f
