"""Mesh simplification on the device: vertex clustering with quadric-error placement (csrc/ofx_simplify.hip;
Lindstrom 2000).  The reference has no counterpart -- its users decimate the OBJ files of export_mesh
(models/octfusion_model_union.py:435-468) on the host, with trimesh or meshlab, one mesh at a time.

A uniform grid is laid over each mesh's bounding box; every occupied cell becomes one vertex, placed where the summed
squared distances to the planes of the cell's faces are least (regularised towards the mean of the cell's vertices);
faces that still have three different corners survive, the first of equal ones wins.  The result is a pure function
of the mesh -- bitwise reproducible, the same alone or inside a batch -- and tests/simplify_oracle.py restates it with
numpy.  DESIGN.md section 4.16 gives the rule and how it differs from an edge-collapse decimator (topology can change
where two sheets share a cell; the face count is steered by ``cells``, not set; no attributes).

    python -m octfusion_amd.simplify --input samples --out simple --cells 64
    python -m octfusion_amd.simplify --input a.obj b.obj --out simple --cell-size 0.02 --clean
"""
import argparse
import json
import math
import os

import numpy as np
import torch

from . import _lib, mesh

MAX_CELLS = 1024        # csrc/ofx_simplify.hip: 10 bits per axis of the vertex key
STAT_KEYS = ('clusters', 'faces_collapsed', 'faces_duplicate', 'clusters_unused')
_MAX_FACES = (2 ** 31 - 1) // 3


def _check_args(cells, cell_size, reg):
    if (cells is None) == (cell_size is None):
        raise ValueError('simplify: exactly one of cells and cell_size must be given')
    if cells is not None:
        if isinstance(cells, bool) or int(cells) != cells or not 1 <= cells <= MAX_CELLS:
            raise ValueError('simplify: cells must be an integer in [1, %d], got %r' % (MAX_CELLS, cells))
    else:
        if not (math.isfinite(cell_size) and cell_size > 0):
            raise ValueError('simplify: cell_size must be finite and > 0, got %r' % (cell_size,))
    if not 0 < reg <= 1:
        raise ValueError('simplify: reg must lie in (0, 1], got %r' % (reg,))


def _groups(meshes):
    """mesh._mesh_groups, cut further where the faces of a group would pass the (2^31 - 1) / 3 incidence slots."""
    out = []
    for grp in mesh._mesh_groups(meshes):
        cur, F = [], 0
        for k in grp:
            nf = int(meshes[k][1].shape[0])
            if nf > _MAX_FACES or int(meshes[k][0].shape[0]) >= 2 ** 31 - 1:
                raise ValueError('simplify: shape %d has more than %d faces or 2^31 - 2 vertices' % (k, _MAX_FACES))
            if cur and F + nf > _MAX_FACES:
                out.append(cur)
                cur, F = [], 0
            cur.append(k)
            F += nf
        if cur:
            out.append(cur)
    return out


def _empty_stats():
    return dict.fromkeys(STAT_KEYS, 0)


def _simplify_group(verts, faces, nv, nf, first, cells, cell_size, reg, stages=None):
    """One batch mesh (nv / nf: per-shape counts on the host; first: index of its first shape, for the messages).
    Returns (meshes, stats)."""
    B, V, F = len(nv), sum(nv), sum(nf)
    if F == 0 or V == 0:
        return [(verts[:0], faces[:0]) for _ in range(B)], [_empty_stats() for _ in range(B)]
    dev = faces.device
    st = _lib.stream()
    L = _lib.lib()
    nbytes = L.ofx_simplify_ws_bytes(V, F, B)
    if nbytes == 0:
        raise ValueError('simplify: %d vertices, %d faces outside the limits of one call' % (V, F))
    offs = torch.from_numpy(np.stack([np.concatenate([[0], np.cumsum(nv)]),
                                      np.concatenate([[0], np.cumsum(nf)])]).astype(np.int64)).to(dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(B * 8, dtype=torch.int64, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.call('ofx_simplify_cluster', _lib.ptr(verts), _lib.ptr(faces), _lib.ptr(offs[0]), _lib.ptr(offs[1]), B, V, F,
              int(cells) if cells is not None else 0, float(cell_size) if cell_size is not None else 0.0, float(reg),
              L.ofx_simplify_stages() if stages is None else stages, _lib.ptr(counts), _lib.ptr(ws), _lib.ptr(status),
              st)
    if stages is not None:                             # a timing run of the first stages: nothing to read
        return None, None
    host = torch.cat([counts, status.to(torch.int64)]).cpu()          # the host sync
    bad, over = int(host[-2]), int(host[-1])       # over: bit 0 a grid overflow, bit 1 a non-finite vertex
    c = host[:-2].view(B, 8)
    if bad & 2:
        raise ValueError('simplify: inconsistent offsets')
    if bad:
        raise ValueError('simplify: shape %d has a face index outside [0, V)'
                         % (first + int(torch.nonzero(c[:, 5])[0])))
    if over & 2:
        raise ValueError('simplify: shape %d has a non-finite vertex' % (first + int(torch.nonzero(c[:, 7])[0])))
    if over:
        raise ValueError('simplify: shape %d needs %d or more cells of size %g along an axis'
                         % (first + int(torch.nonzero(c[:, 6])[0]), MAX_CELLS, cell_size))
    kv, kf = c[:, 1], c[:, 2]
    nvo = torch.cumsum(kv, 0) - kv
    nfo = torch.cumsum(kf, 0) - kf
    out_v = torch.empty(max(int(kv.sum()), 1), 3, dtype=torch.float32, device=dev)
    out_f = torch.empty(max(int(kf.sum()), 1), 3, dtype=torch.int32, device=dev)
    new = torch.stack([nvo, nfo]).to(dev)
    _lib.call('ofx_simplify_extract', _lib.ptr(faces), _lib.ptr(offs[0]), _lib.ptr(offs[1]), B, V, F,
              _lib.ptr(new[0]), _lib.ptr(new[1]), _lib.ptr(out_v), _lib.ptr(out_f), _lib.ptr(ws), _lib.ptr(status), st)
    rows = c.tolist()
    stats = [dict(clusters=r[0], faces_collapsed=r[3], faces_duplicate=r[4], clusters_unused=r[0] - r[1])
             if nf[b] else _empty_stats() for b, r in enumerate(rows)]
    out = [(out_v[int(nvo[b]):int(nvo[b] + kv[b])], out_f[int(nfo[b]):int(nfo[b] + kf[b])]) for b in range(B)]
    return out, stats


def simplify(meshes, cells=None, cell_size=None, reg=1e-3, stats=None):
    """Simplify every mesh of ``meshes`` -- ``(verts [V, 3] fp32, faces [F, 3] int32)`` device tensors, as
    ``mesh.marching_cubes`` and ``mesh.largest_component`` return them -- by vertex clustering.  Exactly one of

      * ``cells=N`` (1 .. 1024): N cells along the longest side of each mesh's own bounding box;
      * ``cell_size=s`` (finite, > 0): cells of side s, anchored at the box's minimum corner; a mesh that would need
        1024 or more cells along an axis raises ValueError.

    ``reg`` in (0, 1] pulls a cell's vertex from the minimiser of its quadric towards the mean of its input vertices:
    it bounds the condition number of the 3 x 3 solve by 3 / reg + 1, so flat and edge-like cells need no rank
    threshold.  Returns a list of pairs of the same types: one vertex per cell that a surviving face uses (cells in
    ascending (ix, iy, iz) order), the surviving faces in input order, each rotated so that its lowest vertex comes
    first (winding kept).  A mesh without faces, or whose faces all collapse (``cells=1``), comes back empty.

    ``stats`` (optional dict): ``stats['meshes']`` becomes one dict per mesh of exact integers -- ``clusters``
    (occupied cells), ``faces_collapsed`` (fewer than three different cells), ``faces_duplicate`` (same cells as an
    earlier face, same winding), ``clusters_unused`` (cells no surviving face uses); all zero for a mesh without faces.

    One host synchronisation per group of meshes (the kept counts and the status words; the workspace is sized from V
    and F).  Raises ValueError for a wrong dtype, device or argument before any launch, ValueError naming the shape for
    a face index outside ``[0, V)`` (checked on the device before anything follows an index), a NaN or infinite vertex
    coordinate (whether a face uses the vertex or not, under ``cells`` and ``cell_size`` alike) or a grid overflow,
    after the readback, and OfxError without a GPU (there is no CPU path)."""
    _lib.require_device()
    meshes = mesh._check_meshes(meshes, 'simplify')
    _check_args(cells, cell_size, reg)
    out, per = [], []
    for grp in _groups(meshes):
        part = [meshes[k] for k in grp]
        v, f = mesh._cat(part)
        o, s = _simplify_group(v, f, [int(m[0].shape[0]) for m in part], [int(m[1].shape[0]) for m in part], grp[0],
                               cells, cell_size, reg)
        out += o
        per += s
    if stats is not None:
        stats['meshes'] = per
    return out


def _inputs(paths):
    files = []
    for p in paths:
        if os.path.isdir(p):
            files += [os.path.join(p, n) for n in sorted(os.listdir(p)) if n.endswith('.obj')]
        else:
            files.append(p)
    return files


def main(argv=None):
    ap = argparse.ArgumentParser(description='Simplify OBJ files on the device (vertex clustering, quadric placement).')
    ap.add_argument('--input', nargs='+', required=True, help='OBJ files, or directories of them')
    ap.add_argument('--out', required=True, help='directory of the simplified <name>.obj files')
    ap.add_argument('--cells', type=int, default=None, help='cells along the longest side of each mesh (1 .. 1024)')
    ap.add_argument('--cell-size', type=float, default=None, help='cell side, in the mesh\'s own units')
    ap.add_argument('--reg', type=float, default=1e-3)
    ap.add_argument('--clean', action='store_true', help='keep only the largest component of every mesh first')
    ap.add_argument('--error', type=int, nargs='?', const=100000, default=None, metavar='N',
                    help='add mesh_query.mesh_error(input, output, N) per mesh to the report: how far the surface '
                         'moved, measured exactly against the triangles (N samples per side, default 100000)')
    ap.add_argument('--check', action='store_true',
                    help='print the mesh_check.check report of every output (clustering can leave non-manifold edges '
                         'and folded faces behind), one JSON line each before the result line, which gains "check"')
    args = ap.parse_args(argv)
    if args.error is not None and args.error < 1:
        raise ValueError('simplify: --error needs at least one sample')
    _check_args(args.cells, args.cell_size, args.reg)
    _lib.require_device()
    dev = torch.device('cuda', torch.cuda.current_device())
    files = _inputs(args.input)
    names = [os.path.splitext(os.path.basename(p))[0] for p in files]
    if len(set(names)) != len(names):
        raise ValueError('simplify: two inputs share a file name')
    meshes = []
    for p in files:
        v, f = mesh.read_obj(p)
        meshes.append((torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)))
    before = [(int(v.shape[0]), int(f.shape[0])) for v, f in meshes]
    if args.clean:
        meshes = mesh.largest_component(meshes)
    stats = {}
    out = simplify(meshes, cells=args.cells, cell_size=args.cell_size, reg=args.reg, stats=stats)
    written = []
    for name, (v, f) in zip(names, out):
        written.append(mesh.write_obj(os.path.join(args.out, name + '.obj'), v, f))
    res = {'files': names, 'cells': args.cells, 'cell_size': args.cell_size, 'reg': args.reg, 'clean': args.clean,
           'vertices_in': [b[0] for b in before], 'faces_in': [b[1] for b in before],
           'vertices_out': [int(v.shape[0]) for v, _ in out], 'faces_out': [int(f.shape[0]) for _, f in out],
           'written': written, 'stats': stats['meshes']}
    if args.error is not None:
        from . import mesh_query
        res['error'] = [mesh_query.mesh_error(m, o, args.error) if m[1].shape[0] and o[1].shape[0] else None
                        for m, o in zip(meshes, out)]
    if args.check:
        from . import mesh_check
        res['check'] = mesh_check.reports(zip(names, out))
        for r in res['check']:
            print(json.dumps(r))
    print(json.dumps(res))
    return res


if __name__ == '__main__':
    main()
