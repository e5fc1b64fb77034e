"""The mesh as a graph, and what is done with it before a mesh is handed on: fairing and per-vertex normals.  On the
device (csrc/ofx_meshsmooth.hip), deterministic, batched like ``mesh_check``.

* ``adjacency``       per mesh the neighbour rows (CSR) and the vertex flags: used / boundary / non-manifold.
* ``vertex_normals``  area-, angle- or uniformly weighted, fp64 sums in a fixed order, fp32 out.
* ``smooth``          Laplacian or Taubin (lambda | mu) fairing, uniform or cotangent weights, the boundary fixed,
                      sliding along itself or free.  The state is fp64 for the whole call and rounded once.

    python -m octfusion_amd.mesh_smooth --input A.obj [B.obj ...] --out DIR [--iterations K] [--lambda L]
        [--mu M | --laplacian] [--weights uniform|cot] [--boundary fixed|slide|free] [--normals [area|angle|uniform]]

The exact rules are in include/ofx.h; tests/smooth_oracle.py restates them in numpy float64.  Nothing is repaired: run
``mesh_check.weld`` first on a file that repeats its vertices, or every face is an island.  There is no CPU path.
"""
import argparse
import json
import math
import os

import torch

from . import _lib, mesh
from ._lib import call, ptr, stream
from .mesh_check import _gather, _mesh_args, _read, _ws, to_device

NORMAL_MODES = {'area': 0, 'angle': 1, 'uniform': 2}
WEIGHTS = {'uniform': 0, 'cot': 1}
BOUNDARY = {'fixed': 0, 'slide': 1, 'free': 2}
MAX_ITERATIONS = 10000


def _choice(table, value, who, what):
    if value not in table:
        raise ValueError('%s: %s %r is not one of %s' % (who, what, value, ', '.join(sorted(table))))
    return table[value]


def adjacency(meshes, corners=False):
    """Per mesh of ``meshes`` (``(verts [V, 3] fp32, faces [F, 3] int32)`` device tensors) ``(row_off [V + 1] int64,
    nbr int32, vflags [V] int32)``: row i of ``nbr`` is ``nbr[row_off[i]:row_off[i + 1]]``, the distinct vertices that
    share a face with vertex i, ascending; ``vflags`` bit 0: a face uses the vertex, bit 1: it lies on an edge with
    one face (boundary), bit 2: on an edge with three or more.  Faces with fewer than three different indices take no
    part.  ``corners=True`` adds ``(corner_off [V + 1] int64, corner int32)``: the corners ``3 face + k`` at every
    vertex, ascending.  One sort, one scan; one host read (the row offsets).  Raises ValueError naming the mesh for a
    mesh without faces, a face index outside ``[0, V)`` or a non-finite vertex used by a face."""
    _lib.require_device()
    who = 'adjacency'
    g = _gather(meshes, who)
    B, V, F, dev = g['B'], sum(g['nv']), sum(g['nf']), g['dev']
    ws = _ws(g, 'ofx_mesh_adjacency_ws_bytes', who)
    row_off = torch.empty(V + 1, dtype=torch.int64, device=dev)
    nbr = torch.empty(6 * F, dtype=torch.int32, device=dev)
    vflags = torch.empty(V, dtype=torch.int32, device=dev)
    corner_off = torch.empty(V + 1, dtype=torch.int64, device=dev) if corners else None
    corner = torch.empty(3 * F, dtype=torch.int32, device=dev) if corners else None
    status = torch.empty(B, dtype=torch.int32, device=dev)
    call('ofx_mesh_adjacency', *_mesh_args(g), V, F, ptr(row_off), ptr(nbr), ptr(vflags), ptr(corner_off), ptr(corner),
         ptr(ws), ptr(status), stream())
    host = _read(g, status, who, row_off, *([corner_off] if corners else []))          # the host read
    lists = [(row_off, nbr, host[0])] + ([(corner_off, corner, host[1])] if corners else [])
    out, v0 = [], 0
    for b in range(B):
        v1 = v0 + g['nv'][b]
        cut = [(off[v0:v1 + 1] - int(h[v0]), vals[int(h[v0]):int(h[v1])]) for off, vals, h in lists]
        out.append((cut[0][0], cut[0][1], vflags[v0:v1]) + (cut[1] if corners else ()))
        v0 = v1
    return out


def vertex_normals(meshes, weight='angle'):
    """Per mesh the unit vertex normals ``[V, 3]`` fp32: the sum over the corners at a vertex, in corner order and in
    fp64, of the face's ``(b - a) x (c - a)`` (``'area'``), of its unit normal (``'uniform'``) or of its unit normal
    times the corner's angle (``'angle'``, the default: the one that does not depend on how a flat region is
    triangulated), normalised and rounded once.  A face without area adds nothing; a vertex no face uses, or whose
    terms cancel, gets (0, 0, 0).  One host read (the status words).  Raises ValueError as ``adjacency`` does."""
    _lib.require_device()
    who = 'vertex_normals'
    mode = _choice(NORMAL_MODES, weight, who, 'weight')
    g = _gather(meshes, who)
    B, V, F, dev = g['B'], sum(g['nv']), sum(g['nf']), g['dev']
    ws = _ws(g, 'ofx_mesh_vertex_normals_ws_bytes', who)
    normals = torch.empty(V, 3, dtype=torch.float32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    call('ofx_mesh_vertex_normals', *_mesh_args(g), V, F, mode, ptr(normals), ptr(ws), ptr(status), stream())
    _read(g, status, who)                                                              # the host read
    return list(normals.split(g['nv']))


def smooth(meshes, iterations=10, lam=0.5, mu=-0.53, weights='uniform', boundary='fixed', dtype=torch.float32):
    """Fair every mesh of ``meshes``: a list of ``(verts, faces)`` with ``faces`` the input tensor itself and ``verts``
    of ``dtype`` (float32, or float64 for the unrounded state).

    One iteration moves every vertex towards the weighted mean of its neighbours by ``lam`` (0 < lam <= 1) and then,
    unless ``mu`` is None (plain Laplacian, which shrinks), by ``mu`` < 0 (Taubin: with mu a little beyond -lam the
    pair is a low-pass filter that keeps the volume).  ``weights``: ``'uniform'`` or ``'cot'`` (cotangent weights of
    the INPUT mesh, negative ones clamped to 0, kept for all iterations).  ``boundary``: ``'fixed'`` (vertices on an
    edge with one face keep their bits), ``'slide'`` (they average only their neighbours along the boundary) or
    ``'free'``.  Faces with fewer than three different indices take no part; vertices no face uses keep their bits.
    fp64 state, sums in a fixed order, rounded once: bitwise reproducible, alone or in a batch.  One host read (the
    status words).  Raises ValueError for arguments out of range before anything is launched, and naming the mesh
    for a mesh without faces, a face index outside ``[0, V)`` or a non-finite vertex used by a face."""
    who = 'smooth'
    iterations = int(iterations)
    if not 0 <= iterations <= MAX_ITERATIONS:
        raise ValueError('%s: iterations %d outside [0, %d]' % (who, iterations, MAX_ITERATIONS))
    lam = float(lam)
    if not 0.0 < lam <= 1.0:
        raise ValueError('%s: lam %r outside (0, 1]' % (who, lam))
    if mu is not None:
        mu = float(mu)
        if not (math.isfinite(mu) and mu < 0.0):
            raise ValueError('%s: mu %r is neither None nor a finite negative number' % (who, mu))
    wmode = _choice(WEIGHTS, weights, who, 'weights')
    bmode = _choice(BOUNDARY, boundary, who, 'boundary')
    if dtype not in (torch.float32, torch.float64):
        raise ValueError('%s: dtype must be torch.float32 or torch.float64' % who)
    _lib.require_device()
    g = _gather(meshes, who)
    B, V, F, dev = g['B'], sum(g['nv']), sum(g['nf']), g['dev']
    ws = _ws(g, 'ofx_mesh_smooth_ws_bytes', who, wmode)
    out = torch.empty(V, 3, dtype=torch.float32, device=dev)
    out64 = torch.empty(V, 3, dtype=torch.float64, device=dev) if dtype == torch.float64 else None
    status = torch.empty(B, dtype=torch.int32, device=dev)
    call('ofx_mesh_smooth', *_mesh_args(g), V, F, wmode, bmode, lam, 0.0 if mu is None else mu, iterations, ptr(out),
         ptr(out64), ptr(ws), ptr(status), stream())
    _read(g, status, who)                                                              # the host read
    vs = (out if out64 is None else out64).split(g['nv'])
    return [(vs[b], m[1]) for b, m in enumerate(meshes)]


def parser():
    ap = argparse.ArgumentParser(prog='python -m octfusion_amd.mesh_smooth', description=__doc__.split('\n\n')[0])
    ap.add_argument('--input', required=True, nargs='+', metavar='OBJ')
    ap.add_argument('--out', required=True, metavar='DIR', help='the smoothed meshes go to DIR/<name of the input>')
    ap.add_argument('--iterations', type=int, default=10)
    ap.add_argument('--lambda', dest='lam', type=float, default=0.5)
    ap.add_argument('--mu', type=float, default=-0.53)
    ap.add_argument('--laplacian', action='store_true', help='no mu step: plain Laplacian smoothing (it shrinks)')
    ap.add_argument('--weights', choices=sorted(WEIGHTS), default='uniform')
    ap.add_argument('--boundary', choices=sorted(BOUNDARY), default='fixed')
    ap.add_argument('--normals', nargs='?', const='angle', default=None, choices=sorted(NORMAL_MODES),
                    help='also write vn lines: the vertex normals of the smoothed mesh (default weight: angle)')
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    _lib.require_device()
    meshes = [to_device(mesh.read_obj(p)) for p in args.input]
    res = smooth(meshes, iterations=args.iterations, lam=args.lam, mu=None if args.laplacian else args.mu,
                 weights=args.weights, boundary=args.boundary)
    normals = vertex_normals(res, weight=args.normals) if args.normals else [None] * len(res)
    rows = []
    for p, (v, f), n in zip(args.input, res, normals):
        dst = os.path.join(args.out, os.path.basename(p))
        mesh.write_obj(dst, v, f, normals=n)
        rows.append(dict(name=p, out=dst, vertices=int(v.shape[0]), faces=int(f.shape[0])))
        print(json.dumps(rows[-1]))
    return rows


if __name__ == '__main__':
    main()
