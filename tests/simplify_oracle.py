"""numpy restatement of the vertex-clustering rule of csrc/ofx_simplify.hip (octfusion_amd.simplify.simplify; DESIGN.md
section 4.16).  float64 throughout; the output positions are rounded once to fp32.

  1. grid      lo / hi = exact per-axis min / max of ALL vertices, side = max axis of hi - lo; h = side / cells or
               h = cell_size; cell = floor((v - lo) / h) per axis, clamped to cells - 1 under `cells`, an index >= 1024
               an error under `cell_size`; side == 0: everything in cell (0, 0, 0).  A NaN or infinite coordinate in
               ANY vertex (used by a face or not) is an error in both modes (`nonfinite`).
  2. clusters  one per occupied cell, numbered in ascending (ix, iy, iz); m = mean of its vertices (summed in ascending
               vertex id); c = lo + (cell + 0.5) h.
  3. quadrics  face (p0, p1, p2), once for each distinct cluster k among its corners: q_i = p_i - c_k,
               n = (q1 - q0) x (q2 - q0), A_k += n n^T, b_k += (n . q0) n.
  4. placement lam = reg trace(A) / 3; trace == 0: x = m; else (A + lam I) y = b + lam (m - c),
               x = clamp(y + c, the cell's box); then fp32.
  5. faces     corners -> clusters; dropped unless the three differ (faces_collapsed); rotated so that the lowest
               cluster comes first; dropped if an earlier face has the same rotated triple (faces_duplicate).
  6. compact   clusters no surviving face uses are dropped (clusters_unused), the rest renumbered in order.
"""
import numpy as np

MAX_CELLS = 1024


def nonfinite(verts):
    """True iff a coordinate of any vertex is NaN or infinite: the device flags the shape (status[1] bit 1, counts
    column 7) and simplify raises."""
    return not bool(np.isfinite(np.asarray(verts, np.float32)).all())


def grid(verts, cells=None, cell_size=None):
    """(lo [3], h, cell [V, 3] int64) of one mesh's vertices."""
    if (cells is None) == (cell_size is None):
        raise ValueError('exactly one of cells and cell_size')
    if nonfinite(verts):
        raise ValueError('non-finite vertex')
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    side = float((hi - lo).max())
    h = side / cells if cells is not None else float(cell_size)
    if side == 0.0:
        cell = np.zeros(v.shape, np.int64)
    else:
        cell = np.floor((v - lo) / h).astype(np.int64)
        if cells is not None:
            cell = np.minimum(cell, cells - 1)
        elif cell.max() >= MAX_CELLS:
            raise ValueError('grid overflow: cell_size needs %d cells' % (cell.max() + 1))
    return lo, h, cell


def rotate(tri):
    """Rows rotated so that the lowest entry comes first (winding kept)."""
    r = np.argmin(tri, 1)
    j = (r[:, None] + np.arange(3)[None, :]) % 3
    return np.take_along_axis(tri, j, 1)


def simplify(verts, faces, cells=None, cell_size=None, reg=1e-3, detail=None):
    """(verts' [V', 3] float32, faces' [F', 3] int32, stats) of one mesh.  stats: clusters, faces_collapsed,
    faces_duplicate, clusters_unused.  detail (optional dict) receives lo, h, the cells and the float64 positions of
    the kept clusters."""
    v32 = np.ascontiguousarray(np.asarray(verts, np.float32).reshape(-1, 3))
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    stats = dict(clusters=0, faces_collapsed=0, faces_duplicate=0, clusters_unused=0)
    if len(f) == 0 or len(v32) == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), stats
    if f.min() < 0 or f.max() >= len(v32):
        raise ValueError('face index outside [0, V)')
    v = v32.astype(np.float64)
    lo, h, cell = grid(v32, cells, cell_size)
    key = (cell[:, 0] << 20) | (cell[:, 1] << 10) | cell[:, 2]
    ukey, cid = np.unique(key, return_inverse=True)
    K = len(ukey)
    ucell = np.stack([ukey >> 20, (ukey >> 10) & 1023, ukey & 1023], 1)
    cnt = np.bincount(cid, minlength=K)
    m = np.zeros((K, 3))
    np.add.at(m, cid, v)                                   # ascending vertex id
    m /= cnt[:, None]
    c = lo + (ucell + 0.5) * h

    # quadrics: one (cluster, face) incidence for each distinct cluster among a face's corners
    fc = cid[f]                                            # [F, 3]
    first = np.ones(fc.shape, bool)
    first[:, 1] = fc[:, 1] != fc[:, 0]
    first[:, 2] = (fc[:, 2] != fc[:, 0]) & (fc[:, 2] != fc[:, 1])
    ft, fj = np.nonzero(first)
    k = fc[ft, fj]
    q = v[f[ft]] - c[k][:, None, :]                        # [I, 3, 3]
    n = np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])
    A = np.zeros((K, 3, 3))
    b = np.zeros((K, 3))
    np.add.at(A, k, n[:, :, None] * n[:, None, :])
    np.add.at(b, k, (n * q[:, 0]).sum(1)[:, None] * n)

    tr = A[:, 0, 0] + A[:, 1, 1] + A[:, 2, 2]
    x = m.copy()
    s = tr != 0
    if s.any():
        lam = reg * tr[s] / 3.0
        M = A[s] + lam[:, None, None] * np.eye(3)
        rhs = b[s] + lam[:, None] * (m[s] - c[s])
        y = np.linalg.solve(M, rhs[:, :, None])[:, :, 0]
        x[s] = np.clip(y + c[s], lo + ucell[s] * h, lo + (ucell[s] + 1) * h)

    distinct = (fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 0] != fc[:, 2])
    kept = np.nonzero(distinct)[0]
    tri = rotate(fc[kept])
    _, firsts = np.unique(tri, axis=0, return_index=True)  # index of the first occurrence of every triple
    firsts = np.sort(firsts)
    tri = tri[firsts]
    used = np.zeros(K, bool)
    used[tri.reshape(-1)] = True
    new = np.cumsum(used) - 1
    stats = dict(clusters=int(K), faces_collapsed=int(len(f) - len(kept)),
                 faces_duplicate=int(len(kept) - len(firsts)), clusters_unused=int(K - used.sum()))
    if detail is not None:
        detail.update(lo=lo, h=h, cell=ucell[used], x64=x[used], cluster_of_vert=cid)
    return x[used].astype(np.float32), new[tri].astype(np.int32).reshape(-1, 3), stats
