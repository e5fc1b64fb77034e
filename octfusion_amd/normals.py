"""Oriented normals for raw point clouds, on the device (csrc/ofx_normals.hip): the stage between "a
point cloud" and the octree build, for scans, depth-fusion results and the ``<index>.npy`` clouds of
``generate.py --points``.

* ``knn``               exact k nearest neighbours of every point inside its own cloud (``ofx_knn``): a uniform grid
                        per cloud, shells of cells searched until the k-th distance rules the rest out.
* ``estimate_normals``  kNN -> per-point PCA in fp64 (``ofx_pca_normals``) -> a consistent outward sign from a
                        volumetric flood of the cloud's exterior, a short march along +-n and a few neighbour votes
                        (``ofx_orient_normals``).

Clouds are [n, 3] tensors on the device, a list of them (a ragged batch, one launch sequence for all) or a ``Points``.
tests/normals_oracle.py restates the three contracts in numpy.  There is no CPU path.

    python -m octfusion_amd.normals --input scan.npy cloud.ply --out DIR [--k 16]

writes DIR/<name>/pointcloud.npz (points, normals) and DIR/<name>/input.ply for ``reconstruct``.
"""
import argparse
import math
import os

import numpy as np
import torch

from . import _lib

MAX_K = 64
MIN_GRID, MAX_GRID = 8, 128
COUNTS = ('undecided_after_march', 'flipped_by_vote', 'undecided', 'degenerate')


def _clouds(points, who):
    """(list of [n_i, 3] float32 contiguous device tensors, the input was a single cloud)."""
    from .octree import Points
    single = not isinstance(points, (list, tuple))
    out = []
    for k, x in enumerate([points] if single else points):
        if isinstance(x, Points):
            x = x.points
        if not torch.is_tensor(x):
            raise TypeError('%s: cloud %d is %s, not a tensor or Points' % (who, k, type(x).__name__))
        if x.device.type != 'cuda':
            raise _lib.OfxError('%s: cloud %d is on %s: octfusion_amd has no CPU path' % (who, k, x.device))
        if x.dim() != 2 or x.shape[1] != 3:
            raise ValueError('%s: cloud %d must be [n, 3], got %s' % (who, k, tuple(x.shape)))
        out.append(x.to(torch.float32).contiguous())
    if not single and not out:
        raise ValueError('%s: an empty list of clouds' % who)
    if len({x.device for x in out}) > 1:
        raise ValueError('%s: the clouds are on different devices' % who)
    return out, single


class _Batch:
    """The concatenated form the entry points take."""

    def __init__(self, clouds):
        self.sizes = [int(x.shape[0]) for x in clouds]
        self.dev = clouds[0].device
        self.total, self.max_n, self.batch = sum(self.sizes), max(self.sizes), len(clouds)
        self.p = torch.cat(clouds).contiguous()
        self.off_host = np.cumsum([0] + self.sizes).tolist()
        self.off = torch.tensor(self.off_host, dtype=torch.int64).to(self.dev)


def _knn(B, k, cells):
    k, cells = int(k), int(cells)
    if not 1 <= k <= MAX_K:
        raise ValueError('knn: k must be in [1, %d], got %d' % (MAX_K, k))
    if cells < 0:
        raise ValueError('knn: cells must be >= 0')
    idx = torch.empty(B.total, k, dtype=torch.int32, device=B.dev)
    d2 = torch.empty(B.total, k, dtype=torch.float32, device=B.dev)
    if B.total:
        nbytes = _lib.lib().ofx_knn_ws_bytes(B.batch, B.total, B.max_n, cells)
        if not nbytes:
            raise ValueError('knn: %d clouds, %d points, cells %d: out of range' % (B.batch, B.total, cells))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=B.dev)
        with torch.cuda.device(B.dev):
            _lib.call('ofx_knn', _lib.ptr(B.p), _lib.ptr(B.off), B.batch, B.total, B.max_n, k, cells, _lib.ptr(ws),
                      _lib.ptr(idx), _lib.ptr(d2), _lib.stream())
    return idx, d2


def knn(points, k, cells=0):
    """Exact k nearest neighbours inside each cloud.  Returns (idx, d2): per cloud idx [n, k] int32 and d2 [n, k]
    float32, rows ascending by (d2, idx) with the point itself a candidate; a cloud of fewer than k points fills the
    rest with (-1, +inf).  d2 = fma(dz, dz, fma(dy, dy, dx * dx)) from direct fp32 differences.  cells: 0 = a grid
    chosen per cloud, c >= 1 = c^3 cells for every cloud (1: the brute-force sweep); the result is bitwise the same for
    every value, alone or in a batch.  Tensors for one cloud, lists for a list."""
    _lib.require_device()
    clouds, single = _clouds(points, 'knn')
    B = _Batch(clouds)
    idx, d2 = _knn(B, k, cells)
    if single:
        return idx, d2
    return list(idx.split(B.sizes)), list(d2.split(B.sizes))


def _cubes(B, d2, k, grid):
    """Per cloud the bounding cube (lo [batch, 3], e [batch] float32 on the device) and the grid size G (host list):
    the cube is centred on the box centre with side e = the largest extent (1 for a cloud without extent); with
    grid=None, G = clamp(floor(e / r), 8, 128) with r the mean distance to the neighbour of rank min(k, 16) - 1.  One
    host read."""
    rank = min(k, 16) - 1
    rows = []
    for b, x in enumerate(B.p.split(B.sizes)):
        if x.shape[0] == 0:
            rows.append(torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0], dtype=torch.float64, device=B.dev))
            continue
        mn, mx = x.min(0).values, x.max(0).values
        e = (mx - mn).max()
        e = torch.where(e > 0, e, torch.ones_like(e))
        lo = (mn + mx) * 0.5 - e * 0.5
        r = d2[B.off_host[b]:B.off_host[b + 1], rank].double().sqrt()
        r = r[torch.isfinite(r)]
        rbar = r.mean() if r.shape[0] else torch.zeros((), dtype=torch.float64, device=B.dev)
        rows.append(torch.cat([lo.double(), e.double().reshape(1), rbar.reshape(1)]))
    rows = torch.stack(rows)
    host = rows.tolist()                                      # the one host read
    G = []
    for b, (_, _, _, e, rbar) in enumerate(host):
        if grid is not None:
            g = int(grid[b] if isinstance(grid, (list, tuple)) else grid)
            if not MIN_GRID <= g <= MAX_GRID:
                raise ValueError('estimate_normals: grid must be in [%d, %d], got %d' % (MIN_GRID, MAX_GRID, g))
        else:
            g = auto_grid(e, rbar)
        G.append(g)
    return rows[:, :3].float().contiguous(), rows[:, 3].float().contiguous(), G, host


def auto_grid(e, rbar):
    """G = clamp(floor(e / rbar), 8, 128); 8 when rbar is 0 or not finite (a cloud of coincident points)."""
    if not (rbar > 0 and math.isfinite(rbar) and math.isfinite(e)):
        return MIN_GRID
    return int(min(max(math.floor(e / rbar), MIN_GRID), MAX_GRID))


def estimate_normals(points, k=16, orient=True, grid=None, steps=8, rounds=3, stats=None, return_variation=False,
                     cells=0):
    """Normals of raw point clouds.  points: an [n, 3] device tensor, a list of such (ragged batch) or a ``Points``.

    kNN (k neighbours, the point itself included) -> PCA: the eigenvector of the smallest eigenvalue of the fp64
    covariance of the neighbours, signed so that its largest component is positive; a point with fewer than 3
    neighbours or a zero covariance gets (0, 0, 0) and counts as degenerate.  orient: give every cloud a consistent
    outward sign.  A grid of G^3 cells over the cloud's bounding cube (grid: an int, one per cloud, or None = from the
    neighbour spacing, 8..128) is flooded from outside; a point marches ``steps`` cells along +n and -n in half-cell
    steps and takes the side that reaches the exterior first; ``rounds`` rounds of neighbour votes settle the rest; a
    sign still undecided stays at the PCA sign.  Thin features below about two cells, thin plates and closed cavities
    are beyond it: DESIGN.md 4.18.

    stats: a dict that receives, per cloud (lists), ``G``, ``lo``, ``e`` (the cube, fp32 values) and the counts
    undecided_after_march, flipped_by_vote, undecided, degenerate, and ``sign`` = the final sign of every point (int8
    device tensors: +1 / -1 as decided, 0 = undecided, kept at the PCA sign).  Without orient G, lo, e and sign are None
    and only degenerate is filled.  Returns the normals ([n, 3] float32; a list for a list), with return_variation also the
    surface variation l0 / (l0 + l1 + l2) per point.  cells: the search grid of ``knn`` (the result does not depend on
    it).  One host read per call."""
    _lib.require_device()
    clouds, single = _clouds(points, 'estimate_normals')
    k, steps, rounds = int(k), int(steps), int(rounds)
    if not 1 <= steps <= 64 or not 0 <= rounds <= 64:
        raise ValueError('estimate_normals: steps must be in [1, 64] and rounds in [0, 64]')
    if isinstance(grid, (list, tuple)) and len(grid) != len(clouds):
        raise ValueError('estimate_normals: %d grid sizes for %d clouds' % (len(grid), len(clouds)))
    B = _Batch(clouds)
    idx, d2 = _knn(B, k, cells)
    nrm = torch.zeros(B.total, 3, dtype=torch.float32, device=B.dev)
    var = torch.zeros(B.total, dtype=torch.float32, device=B.dev)
    degen = torch.zeros(B.batch, dtype=torch.int32, device=B.dev)
    counts = torch.zeros(B.batch, 4, dtype=torch.int32, device=B.dev)
    G = lo_h = e_h = None
    sign = torch.zeros(B.total, dtype=torch.int8, device=B.dev)
    if B.total:
        with torch.cuda.device(B.dev):
            _lib.call('ofx_pca_normals', _lib.ptr(B.p), _lib.ptr(B.off), _lib.ptr(idx), B.batch, B.total, B.max_n, k,
                      _lib.ptr(nrm), _lib.ptr(var), _lib.ptr(degen), _lib.stream())
            if orient:
                lo, e, G, host = _cubes(B, d2, k, grid)
                lo_h, e_h = [r[:3] for r in host], [r[3] for r in host]
                g_dev = torch.tensor(G, dtype=torch.int32).to(B.dev)
                ws = torch.empty(_lib.lib().ofx_orient_normals_ws_bytes(B.batch, B.total, max(G)), dtype=torch.uint8,
                                 device=B.dev)
                out = torch.empty_like(nrm)
                _lib.call('ofx_orient_normals', _lib.ptr(B.p), _lib.ptr(nrm), _lib.ptr(B.off), _lib.ptr(idx), B.batch,
                          B.total, B.max_n, k, _lib.ptr(lo), _lib.ptr(e), _lib.ptr(g_dev), max(G), steps, rounds,
                          _lib.ptr(ws), _lib.ptr(out), _lib.ptr(sign), _lib.ptr(counts), _lib.stream())
                nrm = out
    if stats is not None:
        if orient and B.total:
            c = counts.tolist()
        else:
            c = [[0, 0, 0, d] for d in degen.tolist()]
        stats.update(G=G, lo=lo_h, e=e_h, sign=list(sign.split(B.sizes)) if orient else None)
        for j, name in enumerate(COUNTS):
            stats[name] = [int(row[j]) for row in c]
    if single:
        return (nrm, var) if return_variation else nrm
    nrm, var = list(nrm.split(B.sizes)), list(var.split(B.sizes))
    return (nrm, var) if return_variation else nrm


# ------------------------------------------------------------------------------------------------------------ CLI
def read_cloud(path):
    """points [n, 3] float32 (numpy) of a ``.npy``, a ``.npz`` with the key ``points`` or a PLY (mesh.read_ply)."""
    from . import mesh
    low = path.lower()
    if low.endswith('.npy'):
        pts = np.load(path)
    elif low.endswith('.npz'):
        with np.load(path) as z:
            pts = z['points']
    elif low.endswith('.ply'):
        pts = mesh.read_ply(path)[0]
    else:
        raise ValueError('normals: %s is not a .npy, .npz or .ply file' % path)
    pts = np.ascontiguousarray(pts, np.float32)
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] == 0:
        raise ValueError('normals: %s: points %s, expected [n, 3] with n >= 1' % (path, pts.shape))
    return pts


def parser():
    ap = argparse.ArgumentParser(prog='python -m octfusion_amd.normals', description=__doc__.split('\n\n')[0])
    ap.add_argument('--input', nargs='+', required=True, metavar='FILE', help='.npy, .npz (key points) or .ply clouds')
    ap.add_argument('--out', required=True, metavar='DIR',
                    help='writes DIR/<name>/pointcloud.npz (points, normals) and DIR/<name>/input.ply')
    ap.add_argument('--k', type=int, default=16, help='neighbours per point (1..%d)' % MAX_K)
    return ap


def main(argv=None):
    from . import mesh
    from .reconstruct import shape_name
    args = parser().parse_args(argv)
    names = [shape_name(p) for p in args.input]
    if len(set(names)) != len(names):
        raise ValueError('normals: two inputs share a name')
    clouds = [read_cloud(p) for p in args.input]
    _lib.require_device()
    dev = torch.device('cuda', torch.cuda.current_device())
    stats = {}
    nrm = estimate_normals([torch.from_numpy(c).to(dev) for c in clouds], k=args.k, stats=stats)
    for name, pts, n in zip(names, clouds, nrm):
        d = os.path.join(args.out, name)
        os.makedirs(d, exist_ok=True)
        n = n.cpu().numpy()
        np.savez(os.path.join(d, 'pointcloud.npz'), points=pts, normals=n)
        mesh.write_ply(os.path.join(d, 'input.ply'), pts, n)
    print({key: stats[key] for key in ('G',) + COUNTS})
    return stats


if __name__ == '__main__':
    main()
