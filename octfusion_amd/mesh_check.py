"""Is a triangle mesh sound?  On the device (csrc/ofx_meshcheck.hip): weld equal vertices, report what makes a mesh
closed, manifold and oriented, and find the faces that intersect other faces.

* ``weld``   merge the vertices of a mesh whose three fp32 coordinates are equal (-0 == +0, no tolerance): what a
             ShapeNet-style OBJ that repeats its vertices per face needs before any edge can be counted.
* ``check``  one report per mesh: edges, boundary / non-manifold / inconsistently oriented edges, index-degenerate,
             duplicate and zero-area faces, unreferenced vertices, components, Euler number, genus, area, volume,
             self-intersecting face pairs, and the verdicts ``closed``, ``edge_manifold``, ``oriented``,
             ``watertight``.  ``mesh_to_sdf(signed='auto')`` picks its sign rule from it.

    python -m octfusion_amd.mesh_check --input A.obj [B.obj ...] [--no-weld] [--no-intersections] [--json FILE]

The exact rules are in include/ofx.h; tests/meshcheck_oracle.py restates them in numpy float64.  Not detected: bow-tie
vertices (two fans that share a vertex and no edge).  Nothing is repaired.  There is no CPU path.
"""
import argparse
import json

import numpy as np
import torch

from . import _lib, mesh
from ._lib import call, ptr, stream

COUNTS = ('index_degenerate_faces', 'edges', 'boundary_edges', 'nonmanifold_edges', 'inconsistent_edges',
          'duplicate_faces', 'zero_area_faces', 'unreferenced_vertices', 'components')


def _gather(meshes, who):
    """The checks and the concatenated arrays of one call: verts, faces, offs [2, B + 1] int64 on the device, the host
    lists nv and nf, B, dev."""
    meshes = mesh._check_meshes(meshes, who)
    if not meshes:
        raise ValueError('%s: no meshes' % who)
    B, dev = len(meshes), meshes[0][0].device
    for k, (v, f) in enumerate(meshes):
        if f.shape[0] == 0 or v.shape[0] == 0:
            raise ValueError('%s: shape %d has no faces' % (who, k))
        if v.device != dev:
            raise ValueError('%s: shape %d is on another device' % (who, k))
    if B > 65535:
        raise ValueError('%s: %d shapes exceed one call (65535)' % (who, B))
    return _pack(*mesh._cat(meshes), [int(v.shape[0]) for v, _ in meshes], [int(f.shape[0]) for _, f in meshes], dev)


def _pack(verts, faces, nv, nf, dev):
    offs = torch.from_numpy(np.stack([np.cumsum([0] + nv), np.cumsum([0] + nf)]).astype(np.int64)).to(dev)
    return dict(verts=verts, faces=faces, offs=offs, nv=nv, nf=nf, B=len(nv), dev=dev)


def _ws(g, name, who, *more):
    nbytes = getattr(_lib.lib(), name)(g['B'], sum(g['nv']), sum(g['nf']), *more)
    if nbytes == 0:
        raise ValueError('%s: %d shapes, %d vertices, %d faces out of range' % (who, g['B'], sum(g['nv']), sum(g['nf'])))
    return torch.empty(nbytes, dtype=torch.uint8, device=g['dev'])


def _mesh_args(g):
    return (ptr(g['verts']), ptr(g['faces']), ptr(g['offs'][0]), ptr(g['offs'][1]), g['B'])


def _read(g, status, who, *tensors):
    """The one host read of a pass: int64 tensors and the status words; refuses the first shape the device refused."""
    host = torch.cat([t.reshape(-1).view(torch.int64) for t in tensors] + [status.to(torch.int64)]).cpu()
    bad = torch.nonzero(host[-g['B']:]).flatten().tolist()
    if bad:
        raise ValueError('%s: shape %d has a face index outside [0, %d) or a non-finite vertex used by a face'
                         % (who, bad[0], g['nv'][bad[0]]))
    out, at = [], 0
    for t in tensors:
        out.append(host[at:at + t.numel()].view(t.dtype).reshape(t.shape))
        at += t.numel()
    return out


def _weld(g, who):
    """The welded call of a gathered call and index [V] (old to new).  One host read: the distinct counts."""
    B, V, F, dev = g['B'], sum(g['nv']), sum(g['nf']), g['dev']
    ws = _ws(g, 'ofx_mesh_weld_ws_bytes', who)
    rep = torch.empty(V, dtype=torch.int32, device=dev)
    distinct = torch.empty(B, dtype=torch.int64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    call('ofx_mesh_weld', *_mesh_args(g), V, F, ptr(rep), ptr(distinct), ptr(ws), ptr(status), stream())
    nd = _read(g, status, who, distinct)[0].tolist()                # the host read
    out_v = torch.empty(sum(nd), 3, dtype=torch.float32, device=dev)
    out_f = torch.empty(F, 3, dtype=torch.int32, device=dev)
    index = torch.empty(V, dtype=torch.int32, device=dev)
    call('ofx_mesh_weld_extract', *_mesh_args(g), V, F, ptr(rep), ptr(status), ptr(out_v), ptr(out_f), ptr(index),
         ptr(ws), stream())
    return _pack(out_v, out_f, nd, g['nf'], dev), index, rep


def weld(meshes):
    """Merge the equal vertices of every mesh of ``meshes`` (``(verts [V, 3] fp32, faces [F, 3] int32)`` device
    tensors): a list of ``(verts, faces, index)``.

    Two vertices are equal iff their three coordinates are equal as fp32 values; -0 equals +0; a vertex with a
    non-finite coordinate is never merged.  There is no tolerance.  A group keeps its lowest-indexed vertex with its
    stored bits; the kept vertices stay in their order; ``faces`` are the input's, renumbered -- same count, same
    order, and a face whose corners merged stays (``check`` counts it as index-degenerate); ``index [V]`` int32 maps
    old to new.  Three stable radix sorts and two scans, bitwise reproducible; one host read (the kept counts).
    Raises ValueError naming the mesh for a mesh without faces, a face index outside ``[0, V)`` or a non-finite vertex
    used by a face."""
    _lib.require_device()
    g = _gather(meshes, 'weld')
    w, index, _ = _weld(g, 'weld')
    vs, fs, ix = w['verts'].split(w['nv']), w['faces'].split(w['nf']), index.split(g['nv'])
    return [(vs[k], fs[k], ix[k]) for k in range(g['B'])]


def _topology(g, who, detail):
    B, V, F, dev = g['B'], sum(g['nv']), sum(g['nf']), g['dev']
    ws = _ws(g, 'ofx_mesh_topology_ws_bytes', who)
    counts = torch.empty(B, len(COUNTS), dtype=torch.int64, device=dev)
    sums = torch.empty(B, 2, dtype=torch.float64, device=dev)
    ef = torch.empty(F, 3, dtype=torch.int32, device=dev) if detail else None
    status = torch.empty(B, dtype=torch.int32, device=dev)
    call('ofx_mesh_topology', *_mesh_args(g), V, F, ptr(counts), ptr(sums), ptr(ef), ptr(ws), ptr(status), stream())
    return counts, sums, ef, status


def _selfx(g, bins, who):
    B, F, dev = g['B'], sum(g['nf']), g['dev']
    ws = _ws(g, 'ofx_mesh_selfx_ws_bytes', who, bins)
    partners = torch.empty(F, dtype=torch.int32, device=dev)
    first = torch.empty(F, dtype=torch.int32, device=dev)
    pairs = torch.empty(B, dtype=torch.int64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    call('ofx_mesh_selfx', *_mesh_args(g), max(g['nf']), bins, ptr(partners), ptr(first), ptr(pairs), ptr(ws),
         ptr(status), stream())
    return partners, first, pairs


def check(meshes, weld=True, intersections=True, bins=0, detail=False):
    """One report (a dict) per mesh of ``meshes`` (``(verts, faces)`` device tensors as for ``weld``).

    weld            check the welded mesh (``weld`` above), which is what the counts of a file that repeats its
                    vertices mean; ``welded_vertices`` says how many vertices that removed.  False: the mesh as it is.
    intersections   also search the faces that intersect other faces (``self_intersections`` pairs; None when off).
    bins            the culling grid of that search, as for ``closest_point``: time only, never a bit of the result.
    detail          add the per-face tensors ``edge_faces [F, 3]``, ``partners [F]`` and ``first [F]`` (of the welded
                    mesh's faces, which are the input's in the input's order).

    Counts (include/ofx.h has the exact rules): ``vertices``, ``faces``, ``index_degenerate_faces`` (fewer than three
    different indices; such a face takes part in nothing else), ``edges``, ``boundary_edges`` (one face),
    ``nonmanifold_edges`` (three or more), ``inconsistent_edges`` (two faces walking it the same way),
    ``duplicate_faces``, ``zero_area_faces``, ``unreferenced_vertices``, ``components``.  ``edge_faces[f, k]`` is
    the number of faces on the edge leaving corner k, negative where that edge is inconsistent: where a defect is.
    Derived: ``euler`` = referenced vertices - edges + faces that are not index-degenerate; ``closed`` (no boundary
    edge), ``edge_manifold`` (no non-manifold edge), ``oriented`` (no inconsistent edge); ``watertight`` = closed and
    edge-manifold with no index-degenerate and no duplicate face; ``genus`` = components - euler / 2 when watertight
    and oriented, else None; ``area``, ``volume`` (fp64 sums in a fixed order: bitwise reproducible; the volume
    means something for a closed, oriented mesh).  Two faces intersect when they touch anywhere they do not share
    by index; neighbours only when one is folded flat onto the other.  Bow-tie vertices are not detected.

    Host reads per call, not per mesh: one for the weld's counts, one for everything else.  Raises ValueError naming
    the mesh for a mesh without faces, a face index outside ``[0, V)`` or a non-finite vertex used by a face."""
    _lib.require_device()
    who = 'check'
    bins = int(bins)
    if not 0 <= bins <= mesh.MAX_BINS:
        raise ValueError('%s: bins %d outside [0, %d]' % (who, bins, mesh.MAX_BINS))
    g0 = _gather(meshes, who)
    g = _weld(g0, who)[0] if weld else g0
    counts, sums, ef, status = _topology(g, who, detail)
    partners = first = pairs = None
    if intersections:
        partners, first, pairs = _selfx(g, bins, who)
    host = _read(g, status, who, counts, sums, *([pairs] if intersections else []))      # the host read
    counts, sums = host[0].tolist(), host[1].tolist()
    pairs = host[2].tolist() if intersections else [None] * g['B']
    if any(row[-1] < 0 for row in counts):
        raise _lib.OfxError('%s: the component passes gave up (ofx_mesh_cc_label)' % who)
    out = []
    for b in range(g['B']):
        r = dict(vertices=g['nv'][b], faces=g['nf'][b], welded_vertices=g0['nv'][b] - g['nv'][b])
        r.update(zip(COUNTS, counts[b]))
        live = r['faces'] - r['index_degenerate_faces']
        r['euler'] = (r['vertices'] - r['unreferenced_vertices']) - r['edges'] + live
        r['closed'] = r['boundary_edges'] == 0 and live > 0
        r['edge_manifold'] = r['nonmanifold_edges'] == 0
        r['oriented'] = r['inconsistent_edges'] == 0
        r['watertight'] = (r['closed'] and r['edge_manifold'] and r['index_degenerate_faces'] == 0
                           and r['duplicate_faces'] == 0)
        r['genus'] = (2 * r['components'] - r['euler']) // 2 if r['watertight'] and r['oriented'] else None
        r['area'], r['volume'] = sums[b]
        r['self_intersections'] = pairs[b]
        out.append(r)
    if detail:
        efs = ef.split(g['nf'])
        ps = partners.split(g['nf']) if intersections else [None] * g['B']
        fs = first.split(g['nf']) if intersections else [None] * g['B']
        for b, r in enumerate(out):
            r.update(edge_faces=efs[b], partners=ps[b], first=fs[b])
    return out


def ray_parity_is_sound(report):
    """The rule of ``signed='auto'``: ray parity is right for a watertight mesh without self-intersections."""
    return bool(report['watertight'] and report['self_intersections'] == 0)


def to_device(m, dev=None):
    """``(verts, faces)`` numpy arrays or tensors as the fp32 / int32 device tensors the calls above take."""
    dev = dev or torch.device('cuda', torch.cuda.current_device())
    v, f = m
    v = v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v, np.float32))
    f = f if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(f, np.int64))
    return (v.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous(),
            f.to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous())


def reports(named, **kw):
    """``check`` on ``[(name, (verts, faces)), ...]`` (numpy or tensors): a list of JSON-ready dicts with ``name``
    first.  The meshes go in one call; if it refuses one, each is checked alone and a refused mesh reports
    ``error``."""
    named = list(named)
    try:
        res = check([to_device(m) for _, m in named], **kw)
    except ValueError:
        res = []
        for _, m in named:
            try:
                res += check([to_device(m)], **kw)
            except ValueError as e:
                res.append({'error': str(e)})
    return [dict(name=name, **r) for (name, _), r in zip(named, res)]


def parser():
    ap = argparse.ArgumentParser(prog='python -m octfusion_amd.mesh_check', description=__doc__.split('\n\n')[0])
    ap.add_argument('--input', required=True, nargs='+', metavar='OBJ')
    ap.add_argument('--no-weld', action='store_true', help='check the meshes as they are stored')
    ap.add_argument('--no-intersections', action='store_true', help='skip the search for intersecting faces')
    ap.add_argument('--bins', type=int, default=0, help='culling grid of that search (0: automatic)')
    ap.add_argument('--json', metavar='FILE', help='also write the reports, as one JSON list')
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    _lib.require_device()
    res = reports([(p, mesh.read_obj(p)) for p in args.input], weld=not args.no_weld,
                  intersections=not args.no_intersections, bins=args.bins)
    for r in res:
        print(json.dumps(r))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)
    return res


if __name__ == '__main__':
    main()
