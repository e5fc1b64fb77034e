"""Exact point-to-mesh queries on the device (csrc/ofx_meshquery.hip, ``ofx_mesh_query``): what Kaolin, PyTorch3D,
libigl and trimesh call point-to-mesh distance / closest point, with the search and the arithmetic of ``mesh_to_sdf``.

* ``closest_point``  per query point the distance to the nearest triangle (optionally signed by ray parity), that
                     triangle's index and the closest point on it, for a batch of meshes with ragged query sets in one
                     call.  Meshes may live in any frame.
* ``mesh_error``     how far two meshes are apart: surface samples of each measured exactly against the other's
                     triangles (mean, rms, max per direction, and the Hausdorff distance of the samples).
* ``winding_number`` the generalized winding number of every point around its mesh (csrc/ofx_winding.hip,
                     ``ofx_mesh_winding``): the robust inside / outside of open, self-intersecting or nested meshes.
                     ``occupancy`` is ``w > 0.5``, and ``signed='winding'`` signs the two calls above by it.

    python -m octfusion_amd.mesh_query --a A.obj --b B.obj [--samples N] [--signed [winding]] [--beta B]

tests/meshquery_oracle.py and tests/winding_oracle.py restate the contracts in numpy float64.  There is no CPU path.
"""
import argparse
import json

import numpy as np
import torch

from . import _lib, mesh, metrics
from ._lib import call, ptr, stream

MAX_BINS = mesh.MAX_BINS
DEFAULT_CLI_BETA = 3.0     # the command lines' --beta: DESIGN.md 4.21's table (error below 1e-2, no occupancy flipped)


def _winding_rule(signed, who):
    """True where ``signed`` selects the winding-number sign; any other string is refused."""
    if isinstance(signed, str):
        if signed != 'winding':
            raise ValueError("%s: signed must be False, True or 'winding', got %r" % (who, signed))
        return True
    return False


def _check_beta(beta, who):
    beta = float(beta)
    if not (beta >= 0.0 and beta < float('inf')):
        raise ValueError('%s: beta %r is not a finite number >= 0' % (who, beta))
    return beta


def closest_point(meshes, points, signed=False, bins=0, want_point=True, beta=0.0):
    """Exact nearest triangle of every point of ``points[b]`` on ``meshes[b]``, for all b in one call.

    meshes: a list of B ``(verts [V, 3] fp32, faces [F, 3] int32)`` device tensors, in any frame.  points: a list of B
    ``[n_b, 3]`` fp32 device tensors (ragged; a set may be empty) or one ``[B, n, 3]`` tensor.  Returns a list of B
    ``(dist [n_b] fp32, face [n_b] int32, point [n_b, 3] fp32 or None)``:

      dist   the distance to the nearest point of the nearest triangle: the minimum over all triangles of the fp64
             expression ``mesh_to_sdf`` minimises, so at a lattice point it is that lattice's value, bit for bit.  With
             ``signed`` it is negative where the ray towards -x crosses the surface an odd number of times (the rule of
             ``mesh_to_sdf``: meaningful for a watertight mesh, the parity for an open one); with
             ``signed='winding'`` it is negative where ``winding_number(meshes, points, beta, bins) > 0.5`` instead,
             which is meaningful for open, self-intersecting and nested meshes too (a second call on the same
             arguments and a second host read);
      face   a triangle that attains it -- the lowest index among exact ties, which are the normal case along the
             medial axis and outside a convex vertex or edge;
      point  the closest point on that triangle (``want_point=False``: not computed, None).

    A query with a non-finite coordinate gets NaN, -1, NaN and disturbs nothing else.  ``bins``: the size of the
    culling grid per mesh, 1 .. 16, or 0 for the rule of include/ofx.h; it changes the time, never a bit of the
    result, and neither does the order of the queries or the batch a mesh is in.  One host read, the status words.
    Raises ValueError naming the mesh for a mesh without faces, a face index outside ``[0, V)`` or a non-finite vertex
    used by a face; ValueError for wrong dtypes, shapes or ``bins`` before anything is launched."""
    _lib.require_device()
    who = 'closest_point'
    by_winding = _winding_rule(signed, who)
    beta = _check_beta(beta, who)
    g = mesh._gather(meshes, [('points', 'point sets', points)], bins, who, 'queries')
    B, nq, dev = g['B'], g['nq'], g['dev']
    Q = sum(nq)
    ws = mesh._bins_ws(g, 'ofx_mesh_query_ws_bytes', who, 'queries')
    dist = torch.empty(Q, dtype=torch.float32, device=dev)
    face = torch.empty(Q, dtype=torch.int32, device=dev)
    point = torch.empty(Q, 3, dtype=torch.float32, device=dev) if want_point else None
    status = torch.empty(B, dtype=torch.int32, device=dev)
    offs = g['offs']
    call('ofx_mesh_query', ptr(g['verts']), ptr(g['faces']), ptr(offs[0]), ptr(offs[1]),
         ptr(g['points']) if Q else None, ptr(offs[2]), B, Q, max(nq), g['bins'], 1 if signed and not by_winding else 0,
         ptr(dist) if Q else None, ptr(face) if Q else None, ptr(point) if want_point and Q else None, ptr(ws),
         ptr(status), stream())
    mesh._raise_bad_shape(status, g, who)                       # the host read
    if by_winding and Q:
        dist = torch.where(_winding(g, beta, who) > 0.5, -dist, dist)
    ds, fs = dist.split(nq), face.split(nq)
    ps = point.split(nq) if want_point else [None] * B
    return [(ds[k], fs[k], ps[k]) for k in range(B)]


def _winding(g, beta, who):
    """``ofx_mesh_winding`` on a gathered call: w [Q] fp32 of all the queries, concatenated.  One host read."""
    B, nq = g['B'], g['nq']
    Q = sum(nq)
    ws = mesh._bins_ws(g, 'ofx_mesh_winding_ws_bytes', who, 'queries')
    w = torch.empty(Q, dtype=torch.float32, device=g['dev'])
    status = torch.empty(B, dtype=torch.int32, device=g['dev'])
    offs = g['offs']
    call('ofx_mesh_winding', ptr(g['verts']), ptr(g['faces']), ptr(offs[0]), ptr(offs[1]),
         ptr(g['points']) if Q else None, ptr(offs[2]), B, Q, max(nq), g['bins'], beta, ptr(w) if Q else None, ptr(ws),
         ptr(status), stream())
    mesh._raise_bad_shape(status, g, who)                       # the host read
    return w


def winding_number(meshes, points, beta=0.0, bins=0):
    """The generalized winding number of every point of ``points[b]`` around ``meshes[b]``, for all b in one call: a
    list of B ``[n_b]`` fp32 tensors.  Arguments, checks and errors are ``closest_point``'s.

    For a closed, outward-oriented surface it is 1 inside and 0 outside; nested or overlapping closed parts add up
    (2 where two overlap), an open surface gives a value that falls off smoothly across its holes, and ``w > 0.5``
    stays a sensible inside for meshes where ray parity means nothing (Jacobson et al. 2013).  Each triangle adds its
    signed solid angle / 4 pi (van Oosterom and Strackee's atan2 form, fp64); zero-area triangles add nothing; a
    query with a non-finite coordinate gets NaN.  On the surface itself the value jumps: a query in a face reads the
    mean of both sides.

    beta = 0 (the default): exact, the sum over every triangle in face order -- a pure function of (mesh, point),
    bitwise, whatever the batch, the order of the points or ``bins``.  beta > 0: the first-order far field -- a bin of
    the ``bins``^3 grid whose centre is farther from the point than beta times its radius counts as one dipole
    (include/ofx.h); faster, approximate (about 2e-2 at beta 2, 5e-3 at beta 3 on the test shapes), dependent on
    ``bins`` and ``beta`` but still bitwise reproducible.  One host read, the status words."""
    _lib.require_device()
    who = 'winding_number'
    beta = _check_beta(beta, who)
    g = mesh._gather(meshes, [('points', 'point sets', points)], bins, who, 'queries')
    return list(_winding(g, beta, who).split(g['nq']))


def occupancy(meshes, points, beta=0.0, bins=0):
    """``winding_number(...) > 0.5`` per point: a list of B ``[n_b]`` bool tensors (False for a non-finite point)."""
    _lib.require_device()
    who = 'occupancy'
    beta = _check_beta(beta, who)
    g = mesh._gather(meshes, [('points', 'point sets', points)], bins, who, 'queries')
    return list((_winding(g, beta, who) > 0.5).split(g['nq']))


def _dev_mesh(m, dev):
    v, f = m
    v = v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v, np.float32))
    f = f if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(f, np.int64))
    return (v.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous(),
            f.to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous())


def mesh_error(a, b, n=100000, seed=0, signed=False, beta=0.0):
    """How far mesh ``a`` and mesh ``b`` (``(verts, faces)``, numpy or tensors, in one common frame) are apart: ``n``
    points are drawn on each (``metrics.sample_surface(normalize=False)``, both with shape id 0) and measured EXACTLY
    against the other's triangles, so only the sampled side carries sampling noise.  Returns a dict

      a_to_b, b_to_a   each {'mean', 'rms', 'max'} of the distances of a's samples to b, of b's samples to a
                       (``signed``: of the signed distances -- mean keeps the sign, rms and max use magnitudes --
                       negative inside the other mesh, which must be watertight; ``signed='winding'``: inside by the
                       winding number, ``beta`` as for ``winding_number``, for raw meshes that are not)
      hausdorff        the larger of the two max
      samples          n

    Reductions run in float64 on the device; two host reads (the status words, the six numbers)."""
    _lib.require_device()
    dev = torch.device('cuda', torch.cuda.current_device())
    ma, mb = _dev_mesh(a, dev), _dev_mesh(b, dev)
    pts = metrics.sample_surface([ma, mb], n=int(n), seed=seed, normalize=False, ids=[0, 0])
    res = closest_point([mb, ma], [pts[0].contiguous(), pts[1].contiguous()], signed=signed, want_point=False,
                        beta=beta)
    rows = []
    for d, _, _ in res:
        d = d.double()
        rows.append(torch.stack([d.mean(), (d * d).mean().sqrt(), d.abs().max()]))
    rows = torch.stack(rows).tolist()
    keys = ('mean', 'rms', 'max')
    return {'a_to_b': dict(zip(keys, rows[0])), 'b_to_a': dict(zip(keys, rows[1])),
            'hausdorff': max(rows[0][2], rows[1][2]), 'samples': int(n)}


def parser():
    ap = argparse.ArgumentParser(prog='python -m octfusion_amd.mesh_query', description=__doc__.split('\n\n')[0])
    ap.add_argument('--a', required=True, metavar='A.obj')
    ap.add_argument('--b', required=True, metavar='B.obj')
    ap.add_argument('--samples', type=int, default=100000, help='points drawn on each mesh')
    ap.add_argument('--signed', nargs='?', const=True, default=False, choices=[True, 'winding'], metavar='winding',
                    help="signed distances: alone by ray parity (both meshes watertight), 'winding' by the winding "
                    'number (raw meshes)')
    ap.add_argument('--beta', type=float, default=DEFAULT_CLI_BETA, help='far-field opening of --signed winding '
                    '(0: exact)')
    ap.add_argument('--seed', type=int, default=0)
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    _lib.require_device()
    res = mesh_error(mesh.read_obj(args.a), mesh.read_obj(args.b), args.samples, args.seed, signed=args.signed,
                     beta=args.beta if args.signed == 'winding' else 0.0)
    print(json.dumps(res))
    return res


if __name__ == '__main__':
    main()
