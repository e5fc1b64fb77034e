"""Float64 oracle of the winding-number contract (include/ofx.h, csrc/ofx_winding.hip): numpy only, no project imports
beyond the other oracles, and on purpose NOT the kernel's algorithm.

  exact      ``mesh2sdf_oracle.winding`` (van Oosterom & Strackee, imported, not copied) over the faces whose float64
             ``(b - a) x (c - a)`` is not exactly zero: all pairs at once, numpy's pairwise sums.
  far field  the rule of include/ofx.h restated: the G^3 centroid bins over the mesh's own box, per bin the dipole
             moment N, the area-weighted centre and the radius; a bin is far for a query iff
             ``|centre - q| > beta r`` and then adds ``N . d / (4 pi |d|^3)``, else its faces' exact terms.  Per query
             it also returns the *margin* ``min_k | |centre_k - q| - beta r_k | / (beta r_k)``: where that is not tiny,
             the device (whose moments differ from these in the last bits) takes the same near / far decisions.

The mesh makers and the query sets are ``mesh2sdf_oracle``'s and ``meshquery_oracle``'s.
"""
import numpy as np

import mesh2sdf_oracle as O
import meshquery_oracle as Q

N_QUERIES = 4096
FAR_SETTINGS = [(4, 2.0), (8, 2.0), (4, 3.0)]             # (bins, beta) of the far-field tests


def shapes():
    """The five meshes of the tests, in the order their query sets are drawn."""
    sphere = O.icosphere(3, (0.07, -0.05, 0.03), 0.55)
    V, F = sphere
    keep = V[F].mean(axis=1)[:, 2] < 0.38                   # a cap cut off: open
    soup = O.merge(O.icosphere(3, (-0.2, 0, 0), 0.45), O.icosphere(3, (0.25, 0.05, 0), 0.4), O.box(-0.1, 0.1),
                   O.plate(0.3, 0.0))
    return [('sphere', sphere), ('torus', O.torus(32, 16, 0.5, 0.2, (0.03, 0.02, -0.04))), ('open', (V, F[keep])),
            ('soup', soup), ('plate', O.plate())]


def query_sets(meshes):
    """``meshquery_oracle.query_sets`` on the meshes: 3072 uniform + 1024 near-surface queries each."""
    sets = Q.query_sets(meshes)
    assert all(len(P) == N_QUERIES for P in sets)
    return sets


def _corners(V, F):
    V = np.asarray(V, np.float64)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    return V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]


def with_area(V, F):
    """[m] bool: the faces whose float64 (b - a) x (c - a) has a non-zero component."""
    a, b, c = _corners(V, F)
    return (np.cross(b - a, c - a) != 0).any(axis=1)


def exact(P, V, F):
    """[n] float64 winding number of the mesh around every point: zero-area faces contribute nothing."""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    keep = with_area(V, F)
    if not keep.any():
        return np.zeros(len(np.asarray(P).reshape(-1, 3)))
    return O.winding(P, V, F[keep])


def auto_bins(F, bins=0):
    """The grid rule of include/ofx.h: ``bins``, or the smallest G in 1 .. 16 with 256 G^2 >= F."""
    if bins:
        return bins
    g = 1
    while g < 16 and 256 * g * g < F:
        g += 1
    return g


def bin_of(V, F, G):
    """[m] bin index (x slowest) of every face: its centroid, clamped, in the G^3 grid over the box of the vertices
    the faces use -- float64, in the operation order of the header so that a centroid on a wall falls the same way."""
    a, b, c = _corners(V, F)
    used = np.concatenate([a, b, c])
    lo, ext = used.min(axis=0), used.max(axis=0) - used.min(axis=0)
    mid = ((a + b) + c) * (1.0 / 3.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        f = np.where(ext > 0, np.floor((mid - lo) / np.where(ext > 0, ext, 1.0) * float(G)), 0.0)
    g = np.clip(f, 0, G - 1).astype(np.int64)
    return (g[:, 0] * G + g[:, 1]) * G + g[:, 2]


def moments(V, F, G):
    """Per non-empty bin that holds a face with area, in bin order: (bin, N [3], centre [3], r, faces [k])."""
    a, b, c = _corners(V, F)
    n = np.cross(b - a, c - a)
    keep = (n != 0).any(axis=1)
    bins = bin_of(V, F, G)
    out = []
    for k in np.unique(bins):
        idx = np.nonzero((bins == k) & keep)[0]
        if len(idx) == 0:
            continue
        area = 0.5 * np.linalg.norm(n[idx], axis=1)
        cent = (a[idx] + b[idx] + c[idx]) / 3.0
        centre = (area[:, None] * cent).sum(axis=0) / area.sum()
        corners = np.concatenate([a[idx], b[idx], c[idx]])
        r = np.linalg.norm(corners - centre, axis=1).max()
        out.append((int(k), 0.5 * n[idx].sum(axis=0), centre, float(r), idx))
    return out


def far(P, V, F, bins, beta):
    """(w [n], margin [n], far_share): the far-field value of include/ofx.h at grid size ``bins`` (0: automatic) and
    opening ``beta`` (taken through fp32, as the entry does), the decision margin per query, and the share of
    (query, bin) decisions that were far."""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    beta = float(np.float32(beta))
    assert beta > 0
    w = np.zeros(len(P))
    margin = np.full(len(P), np.inf)
    n_far = n_all = 0
    for _, N, centre, r, idx in moments(V, F, auto_bins(len(F), bins)):
        d = centre[None] - P
        dist = np.linalg.norm(d, axis=1)
        is_far = dist > beta * r
        with np.errstate(divide='ignore', invalid='ignore'):
            dipole = (d @ N) / (4.0 * np.pi * dist ** 3)
        near = ~is_far
        w[is_far] += dipole[is_far]
        if near.any():
            w[near] += O.winding(P[near], V, F[idx])
        margin = np.minimum(margin, np.abs(dist - beta * r) / (beta * r))
        n_far += int(is_far.sum())
        n_all += len(P)
    return w, margin, n_far / max(n_all, 1)
