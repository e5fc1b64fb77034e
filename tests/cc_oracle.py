"""numpy / scipy restatement of the component contract of csrc/ofx_mesh_cc.hip (octfusion_amd.mesh.components,
largest_component): the reference's export_mesh(clean=True), models/octfusion_model_union.py:459-467.

  * two vertices are connected when a face uses both; components are numbered by their lowest vertex id, and only
    components with a face count (a vertex no face uses has component -1);
  * the table holds exact fp32 bounding boxes and exact counts; the box is ordered by bit pattern (`order_key`): -0.0
    lies below +0.0, denormals and the infinities are ordinary values;
  * the winner has the largest max-axis extent, computed in fp32; np.argmax gives a tie to the first component;
  * extraction keeps vertices and faces in their order and renumbers the indices.
"""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import mc_oracle as M


def _renumber(raw, used):
    """Raw component ids -> ids by first appearance among the used items; unused items get -1."""
    out = np.full(len(raw), -1, np.int64)
    idx = np.nonzero(used)[0]
    if len(idx) == 0:
        return out
    _, first, inv = np.unique(raw[idx], return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    out[idx] = rank[inv]
    return out


def labels(nv, faces):
    """comp_of_vert int64 [nv]: components by shared vertex, renumbered by lowest vertex id; -1 for unused vertices."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if nv == 0 or len(f) == 0:
        return np.full(nv, -1, np.int64)
    r = np.concatenate([f[:, 0], f[:, 1]])
    c = np.concatenate([f[:, 1], f[:, 2]])
    g = coo_matrix((np.ones(len(r), np.int8), (r, c)), shape=(nv, nv))
    _, raw = connected_components(g, directed=False)
    used = np.zeros(nv, bool)
    used[f.reshape(-1)] = True
    return _renumber(raw, used)


def labels_by_edge(faces, exactly_two=False):
    """comp_of_face int64 [F] by face adjacency across shared edges, renumbered by first face.  exactly_two=True is
    trimesh's own notion (graph.face_adjacency groups the sorted edges with require_count=2): an edge that four faces
    share connects nothing.  Only used to pin `labels`."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    nf = len(f)
    if nf == 0:
        return np.zeros(0, np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    owner = np.tile(np.arange(nf), 3)
    key = e[:, 0] * (int(f.max()) + 1) + e[:, 1]
    order = np.argsort(key, kind='stable')
    key, owner = key[order], owner[order]
    if exactly_two:
        start = np.nonzero(np.concatenate([[True], key[1:] != key[:-1]]))[0]
        count = np.diff(np.concatenate([start, [len(key)]]))
        link = start[count == 2]
    else:
        link = np.nonzero(key[1:] == key[:-1])[0]
    g = coo_matrix((np.ones(len(link), np.int8), (owner[link], owner[link + 1])), shape=(nf, nf))
    _, raw = connected_components(g, directed=False)
    return _renumber(raw, np.ones(nf, bool))


def same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    return len(pairs) == len(np.unique(a)) == len(np.unique(b))


def refines(fine, coarse):
    """True iff every class of `fine` lies inside one class of `coarse`."""
    pairs = np.unique(np.stack([np.asarray(fine), np.asarray(coarse)], 1), axis=0)
    return len(pairs) == len(np.unique(fine))


def order_key(x):
    """Order-preserving uint32 image of fp32 values, as the device's integer min / max use it: -0.0 below +0.0."""
    u = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def order_value(e):
    e = np.asarray(e, np.uint32)
    u = np.where(e & np.uint32(0x80000000), e ^ np.uint32(0x80000000), ~e).astype(np.uint32)
    return u.view(np.float32)


def table(verts, faces):
    """dict: comp_of_vert [V], comp_of_face [F], bbox_min / bbox_max fp32 [K, 3], n_verts / n_faces int64 [K]."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    cv = labels(len(v), f)
    cf = cv[f[:, 0]] if len(f) else np.zeros(0, np.int64)
    K = int(cv.max()) + 1 if len(cv) else 0
    K = max(K, 0)
    used = cv >= 0
    order = np.argsort(cv[used], kind='stable')
    idx = np.nonzero(used)[0][order]
    nverts = np.bincount(cv[used], minlength=K).astype(np.int64)
    if K:
        start = np.concatenate([[0], np.cumsum(nverts)[:-1]])
        keys = order_key(v[idx])
        bmin = order_value(np.minimum.reduceat(keys, start, axis=0))
        bmax = order_value(np.maximum.reduceat(keys, start, axis=0))
    else:
        bmin = bmax = np.zeros((0, 3), np.float32)
    return dict(comp_of_vert=cv, comp_of_face=cf, bbox_min=bmin.astype(np.float32), bbox_max=bmax.astype(np.float32),
                n_verts=nverts, n_faces=np.bincount(cf, minlength=K).astype(np.int64))


def extents(tab):
    with np.errstate(over='ignore', invalid='ignore'):
        return (tab['bbox_max'] - tab['bbox_min']).astype(np.float32).max(axis=1) if len(tab['n_verts']) else \
            np.zeros(0, np.float32)


def select(tab):
    """The reference's rule: np.argmax of the max-axis extents (first maximum); -1 without components."""
    e = extents(tab)
    return int(np.argmax(e)) if len(e) else -1


def extract(verts, faces, comp, tab=None):
    """(verts, faces) of component `comp`: kept rows in their order, indices renumbered."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    tab = tab or table(v, f)
    kv = tab['comp_of_vert'] == comp
    kf = tab['comp_of_face'] == comp
    new = np.cumsum(kv) - 1
    return v[kv], new[f[kf]].astype(np.int32)


def clean(verts, faces):
    """(verts, faces, number of components) after the reference's clean=True."""
    tab = table(verts, faces)
    w = select(tab)
    if w < 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 0
    v, f = extract(verts, faces, w, tab)
    return v, f, len(tab['n_verts'])


# ---- fields ------------------------------------------------------------------------------------------------------
def two_spheres(R):
    x, y, z = M.lattice_coords(R)
    a = np.sqrt((x + 0.35) ** 2 + (y - 0.01) ** 2 + (z + 0.02) ** 2) - 0.4
    b = np.sqrt((x - 0.55) ** 2 + (y - 0.3) ** 2 + z ** 2) - 0.18
    return np.minimum(a, b).astype(np.float32)


def rod_and_ball(R):
    x, y, z = M.lattice_coords(R)
    rod = np.maximum(np.sqrt((y - 0.5) ** 2 + (z - 0.5) ** 2) - 0.04, np.abs(x) - 0.8)
    ball = np.sqrt(x ** 2 + (y + 0.2) ** 2 + (z + 0.2) ** 2) - 0.45
    return np.minimum(rod, ball).astype(np.float32)


def noisy(R, s):
    g = M.gaussians(R, seed=s)
    n = np.random.default_rng(s).standard_normal((R, R, R))
    return (g + 1.4 * np.abs(g).mean() * n).astype(np.float32)


def tetra_pair(shift=(4.0, 0.0, 0.0)):
    """Two translated copies of a tetrahedron with exactly representable coordinates: equal extents."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    return np.concatenate([v, v + np.asarray(shift, np.float32)]), np.concatenate([f, f + 4]).astype(np.int32)


def strip(n_faces, seed=0, cut=None):
    """A triangle strip of n_faces faces over n_faces + 2 vertices whose ids are a seeded random permutation; with
    `cut`, face `cut` and its neighbour are left out so that the strip falls into two pieces."""
    perm = np.random.default_rng(seed).permutation(n_faces + 2)
    i = np.arange(n_faces)
    f = np.stack([i, i + 1, i + 2], 1)
    if cut is not None:
        f = f[(i != cut) & (i != cut + 1)]
    faces = perm[f].astype(np.int32)
    t = np.arange(n_faces + 2, dtype=np.float32)
    pos = np.stack([t * np.float32(0.5), (np.arange(n_faces + 2) % 2).astype(np.float32), np.zeros_like(t)], 1)
    verts = np.zeros((n_faces + 2, 3), np.float32)
    verts[perm] = pos
    return verts, faces
