"""Rays against meshes on the device (csrc/ofx_raycast.hip, ``ofx_ray_cast``): what trimesh's ``ray.intersects_location``
answers, exactly and bit-reproducibly, with the bins and the discipline of ``mesh_query``.

* ``ray_cast``      per ray the parameter of its first hit, the face, the hit point and the cosine between the face
                    normal and the ray, for a batch of meshes with ragged ray sets in one call.
* ``camera_rays``   the pixel-centre rays of ``render``'s pinhole camera, in 8 x 8 tile order.
* ``ray_images``    depth, face, hit-point and normal maps of meshes from camera poses -- the reference's
                    ``trimesh_ray_tracing`` and ``render_normal_map`` (utils/render/render_utils.py:175-205, 118-137).
* ``virtual_scan``  the oriented partial cloud a depth sensor at some poses would see, optionally noisy: the input
                    ``normals.py`` and ``reconstruct.py`` exist for.

    python -m octfusion_amd.raycast --input A.obj ... --out DIR [--views K] [--size S] [--noise SIGMA] [--normal-maps]

tests/raycast_oracle.py restates the contract in numpy float64.  There is no CPU path.
"""
import argparse
import json
import math
import os

import numpy as np
import torch

from . import _lib, mesh, render
from ._lib import call, ptr, stream

MAX_BINS = mesh.MAX_BINS
TILE = 8


def _gather(meshes, origins, dirs, bins, who='ray_cast'):
    """``mesh._gather`` for rays: the concatenated rays are its ``'origins'`` and ``'directions'``."""
    return mesh._gather(meshes, [('origins', 'sets of origins', origins), ('directions', 'sets of directions', dirs)],
                        bins, who, 'rays')


def _cast(g, tmin, tmax, want_point, want_cos, coherent, who='ray_cast'):
    """ofx_ray_cast on gathered arguments: (t, face, point | None, cos | None), concatenated.  The host read."""
    tmin, tmax = float(tmin), float(tmax)
    if math.isnan(tmin) or math.isnan(tmax):
        raise ValueError('%s: tmin and tmax must not be NaN' % who)
    B, Q, dev = g['B'], sum(g['nq']), g['dev']
    ws = mesh._bins_ws(g, 'ofx_ray_cast_ws_bytes', who, 'rays')
    t = torch.empty(Q, dtype=torch.float32, device=dev)
    face = torch.empty(Q, dtype=torch.int32, device=dev)
    point = torch.empty(Q, 3, dtype=torch.float32, device=dev) if want_point else None
    cosn = torch.empty(Q, dtype=torch.float32, device=dev) if want_cos else None
    status = torch.empty(B, dtype=torch.int32, device=dev)
    offs = g['offs']
    call('ofx_ray_cast', ptr(g['verts']), ptr(g['faces']), ptr(offs[0]), ptr(offs[1]),
         ptr(g['origins']) if Q else None, ptr(g['directions']) if Q else None, ptr(offs[2]), B, Q, max(g['nq']), tmin,
         tmax, g['bins'], 1 if coherent else 0, ptr(t) if Q else None, ptr(face) if Q else None,
         ptr(point) if want_point and Q else None, ptr(cosn) if want_cos and Q else None, ptr(ws), ptr(status),
         stream())
    mesh._raise_bad_shape(status, g, who)                       # the host read
    return t, face, point, cosn


def ray_cast(meshes, origins, dirs, tmin=0.0, tmax=math.inf, bins=0, want_point=True, want_cos=True, coherent=False):
    """The first hit of every ray ``origins[b][i] + t * dirs[b][i]`` on ``meshes[b]``, for all b in one call.

    meshes: a list of B ``(verts [V, 3] fp32, faces [F, 3] int32)`` device tensors, in any frame.  origins, dirs: lists
    of B ``[n_b, 3]`` fp32 device tensors (ragged; a set may be empty) or ``[B, n, 3]`` tensors.  Directions are not
    normalised: ``t`` is in units of ``|dir|``.  Returns a list of B ``(t [n_b] fp32, face [n_b] int32, point [n_b, 3]
    fp32 or None, cos [n_b] fp32 or None)``:

      t      the smallest parameter in ``[tmin, tmax]`` at which the ray meets a triangle (two-sided, watertight along
             shared edges and vertices: include/ofx.h), ``inf`` for a miss;
      face   that triangle -- the lowest index among exact ties, which are the normal case on an edge -- or -1;
      point  the hit point, from the face's vertices (NaN for a miss; ``want_point=False``: None);
      cos    the face's unit normal dotted with the unit direction: negative where the face is met from its front --
             the reference's ``sign`` is its sign (NaN for a miss; ``want_cos=False``: None).

    A ray with a non-finite component or a zero direction gets inf, -1, NaN, NaN and disturbs nothing else.  ``bins``:
    the size of the culling grid per mesh, 1 .. 16, or 0 for the rule of include/ofx.h.  ``coherent``: consecutive rays
    are neighbours already (``camera_rays``) and need no sort.  Neither they, nor the order of the rays, nor the batch a
    mesh is in change a bit of the result.  One host read, the status words.  Raises ValueError naming the mesh for a
    mesh without faces, a face index outside ``[0, V)`` or a non-finite vertex used by a face; ValueError for wrong
    dtypes, shapes or ``bins`` before anything is launched."""
    _lib.require_device()
    g = _gather(meshes, origins, dirs, bins)
    t, face, point, cosn = _cast(g, tmin, tmax, want_point, want_cos, coherent)
    nq, B = g['nq'], g['B']
    ts, fs = t.split(nq), face.split(nq)
    ps = point.split(nq) if want_point else [None] * B
    cs = cosn.split(nq) if want_cos else [None] * B
    return [(ts[k], fs[k], ps[k], cs[k]) for k in range(B)]


def tile_order(size):
    """(perm, inv) int64 numpy: ``perm[k]`` = the row-major pixel index ``y * size + x`` of the k-th pixel in 8 x 8 tile
    order (tiles row-major, pixels row-major inside a tile, edge tiles cut), ``inv`` its inverse permutation."""
    size = int(size)
    y, x = np.divmod(np.arange(size * size, dtype=np.int64), size)
    key = ((y // TILE) * ((size + TILE - 1) // TILE) + x // TILE) * (TILE * TILE) + (y % TILE) * TILE + x % TILE
    perm = np.argsort(key, kind='stable')
    inv = np.empty_like(perm)
    inv[perm] = np.arange(size * size, dtype=np.int64)
    return perm, inv


def camera_rays(pose, size, yfov=render.YFOV):
    """(origins [size^2, 3], dirs [size^2, 3], inv [size^2] int64) device tensors: the rays through the pixel centres of
    ``render``'s pinhole camera at ``pose`` ([4, 4] camera-to-world, rigid: ``render.look_at``; the camera looks down its
    -z, y up, row 0 is the top), in 8 x 8 tile order; ``x[inv]`` puts a per-ray result ``x`` into row-major pixel order.
    A direction is ``R (u, v, -1)`` with ``u = ((x + 0.5) / size * 2 - 1) tan(yfov / 2)``, ``v = (1 - (y + 0.5) / size
    * 2) tan(yfov / 2)``, computed in float64 and rounded once: its component along the view axis is 1, so ``t`` is
    the depth along the view axis."""
    _lib.require_device()
    size = int(size)
    if not 1 <= size <= 4096:
        raise ValueError('camera_rays: size %d outside [1, 4096]' % size)
    p = np.asarray(pose.detach().cpu().numpy() if torch.is_tensor(pose) else pose, np.float64)
    if p.shape != (4, 4):
        raise ValueError('camera_rays: pose must be [4, 4], got %s' % (p.shape,))
    render.camera_rows(p[None])                                # refuses a pose that is not rigid
    dev = render._device()
    perm, inv = _tile_order_dev(size, dev)
    y, x = (perm // size).double(), (perm % size).double()
    th = math.tan(float(yfov) / 2.0)
    n = torch.full((), float(size), dtype=torch.float64, device=dev)       # a device divisor: a true division
    u, v = ((x + 0.5) / n * 2.0 - 1.0) * th, (1.0 - (y + 0.5) / n * 2.0) * th
    R = torch.from_numpy(np.ascontiguousarray(p[:3, :3])).to(dev)
    d = (u[:, None] * R[:, 0] + v[:, None] * R[:, 1]) + (-1.0) * R[:, 2][None]      # each operation rounded on its own
    o = torch.from_numpy(p[:3, 3].astype(np.float32)).to(dev).expand(d.shape[0], 3).contiguous()
    return o, d.float().contiguous(), inv


_TILE_ORDERS = {}


def _tile_order_dev(size, dev):
    key = (int(size), str(dev))
    if key not in _TILE_ORDERS:
        _TILE_ORDERS[key] = tuple(torch.from_numpy(a).to(dev) for a in tile_order(size))
    return _TILE_ORDERS[key]


def _unit_frame(v):
    """``render``'s normalisation of one mesh: (v - bounding-box centre) / largest distance from it, in float64, rounded
    once to fp32.  A mesh without extent keeps its scale."""
    lo, hi = v.min(0).values.double(), v.max(0).values.double()
    c = (lo + hi) * 0.5
    r = (v.double() - c).square().sum(1).max().sqrt()
    r = torch.where(r > 0, r, torch.ones_like(r))
    return ((v.double() - c) / r).float().contiguous()


def _dev_mesh(m, dev):
    v, f = m
    v = v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v, np.float32))
    f = f if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(f, np.int64))
    return (v.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous(),
            f.to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous())


def _view_rays(poses, size):
    """Origins and directions of all views, view-major, each view in tile order, and the inverse permutation."""
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    if len(poses) < 1:
        raise ValueError('raycast: no poses')
    rays = [camera_rays(p, size) for p in poses]
    return torch.cat([r[0] for r in rays]), torch.cat([r[1] for r in rays]), rays[0][2], poses


def ray_images(meshes, poses=None, size=299, normalize=True, bins=0):
    """What camera rays see of every mesh of ``meshes`` (``(verts, faces)`` pairs, numpy or tensors) from every pose of
    ``poses`` ([V, 4, 4] camera-to-world, rigid; None: the 20 FID views of ``render``).  A dict of device tensors:

      depth   [B, V, size, size] fp32     the distance of the hit along the view axis, ``inf`` on the background
      face    [B, V, size, size] int32    the face hit, -1 on the background
      point   [B, V, size, size, 3] fp32  the hit point (NaN on the background), in the frame the rays were cast in
      normal  [B, V, size, size, 3] uint8 the reference's normal encoding, ``(n + 1) / 2 * 255``, of the world-space unit face
                                          normal turned towards the camera, rounded; the background is 255

    normalize: first map each mesh to the unit sphere as ``render`` does, so that a ray image and a rendered image of
    the same mesh show the same view (``point`` is then in that frame).  One host read, the status words."""
    _lib.require_device()
    dev = render._device()
    ms = [_dev_mesh(m, dev) for m in meshes]
    if normalize:
        ms = [(_unit_frame(v) if v.shape[0] else v, f) for v, f in ms]
    org, dr, inv, poses = _view_rays(render.fid_poses() if poses is None else poses, size)
    B, V, S = len(ms), len(poses), int(size)
    g = _gather(ms, [org] * B, [dr] * B, bins, 'ray_images')
    t, face, point, cosn = _cast(g, 0.0, math.inf, True, True, True, 'ray_images')
    tri = g['faces']
    # the world-space unit normal of every hit face, turned towards the camera (against the ray)
    voff = g['offs'][0][:-1].repeat_interleave(V * S * S)
    foff = g['offs'][1][:-1].repeat_interleave(V * S * S)
    hit = face >= 0
    fid = torch.where(hit, face.long() + foff, foff)
    corner = g['verts'].double()[(tri[fid].long() + voff[:, None])]
    n = torch.cross(corner[:, 1] - corner[:, 0], corner[:, 2] - corner[:, 0], dim=1)
    n = n / n.norm(dim=1, keepdim=True)
    n = torch.where((cosn > 0)[:, None], -n, n)
    rgb = ((n + 1.0) * 0.5 * 255.0 + 0.5).floor().clamp(0.0, 255.0).to(torch.uint8)
    rgb = torch.where(hit[:, None], rgb, torch.full_like(rgb, 255))

    def image(x):
        x = x.view(B, V, S * S, *x.shape[1:])
        return x[:, :, inv].reshape(B, V, S, S, *x.shape[3:])
    return dict(depth=image(t), face=image(face), point=image(point), normal=image(rgb))


def virtual_scan(meshes, poses, size=128, noise=0.0, seed=0, bins=0):
    """The oriented partial cloud a depth sensor would record of every mesh of ``meshes`` (``(verts, faces)`` pairs,
    numpy or tensors, in their own frame) from the camera poses ``poses`` ([V, 4, 4], ``render.look_at``) at ``size`` x
    ``size`` pixels: per mesh ``(points [n, 3] fp32, normals [n, 3] fp32)`` on the device -- the first hits of all views,
    in view then row-major pixel order, compacted on the device; every normal is the hit face's unit normal turned
    towards its camera.  noise: the standard deviation of Gaussian noise added along the ray (in the mesh's units), drawn
    from the project's counter hash keyed by ``seed``, the mesh's position in the list and the ray: two runs are
    bit-equal.  Two host reads (the status words, the counts)."""
    _lib.require_device()
    noise = float(noise)
    if not noise >= 0.0:
        raise ValueError('virtual_scan: noise must be >= 0')
    dev = render._device()
    ms = [_dev_mesh(m, dev) for m in meshes]
    org, dr, inv, poses = _view_rays(poses, size)
    B, V, S = len(ms), len(poses), int(size)
    g = _gather(ms, [org] * B, [dr] * B, bins, 'virtual_scan')
    t, face, _, _ = _cast(g, 0.0, math.inf, False, False, True, 'virtual_scan')

    def rows(x):                    # tile order -> row-major pixels within each view: the order of the compacted cloud
        x = x.view(B, V, S * S, *x.shape[1:])
        return x[:, :, inv].reshape(B * V * S * S, *x.shape[3:]).contiguous()
    t, face, org, dr = rows(t), rows(face), rows(g['origins']), rows(g['directions'])
    Q = sum(g['nq'])
    ws = torch.empty(max(1, _lib.lib().ofx_ray_scan_ws_bytes(Q)), dtype=torch.uint8, device=dev)
    points = torch.empty(Q, 3, dtype=torch.float32, device=dev)
    normals = torch.empty(Q, 3, dtype=torch.float32, device=dev)
    out_off = torch.empty(B + 1, dtype=torch.int64, device=dev)
    offs = g['offs']
    call('ofx_ray_scan', ptr(g['verts']), ptr(g['faces']), ptr(offs[0]), ptr(offs[1]), ptr(org), ptr(dr),
         ptr(offs[2]), B, Q, ptr(t), ptr(face), noise, int(seed) & (2 ** 64 - 1), ptr(points), ptr(normals),
         ptr(out_off), ptr(ws), stream())
    cut = out_off.tolist()                                       # the second host read
    return [(points[cut[k]:cut[k + 1]], normals[cut[k]:cut[k + 1]]) for k in range(B)]


def scan_poses(k):
    """[k, 4, 4]: the first ``k`` of ``render``'s 20 FID poses (eyes on the sphere of radius 2.14 around the origin)."""
    k = int(k)
    if not 1 <= k <= 20:
        raise ValueError('raycast: views %d outside [1, 20]' % k)
    return render.fid_poses()[:k]


def parser():
    ap = argparse.ArgumentParser(prog='python -m octfusion_amd.raycast', description=__doc__.split('\n\n')[0])
    ap.add_argument('--input', nargs='+', required=True, metavar='OBJ', help='OBJ files and / or directories of them')
    ap.add_argument('--out', required=True, metavar='DIR', help='writes DIR/<name>.ply (points and normals)')
    ap.add_argument('--views', type=int, default=4, help='how many of the 20 FID view points scan the mesh')
    ap.add_argument('--size', type=int, default=128, help='pixels per side of a view')
    ap.add_argument('--noise', type=float, default=0.0, help='standard deviation of the noise along the ray, in units '
                    'of the mesh scaled to the unit sphere')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--normal-maps', action='store_true', help='also write DIR/view_<j>/<name>.png normal maps')
    return ap


def main(argv=None):
    """Scans every input mesh, scaled to the unit sphere as ``render`` does, from the first ``--views`` FID poses."""
    args = parser().parse_args(argv)
    _lib.require_device()
    files = render._inputs(args.input)
    if not files:
        raise ValueError('raycast: no OBJ files in %s' % args.input)
    dev = render._device()
    poses = scan_poses(args.views)
    counts = {}
    for path in files:
        name = os.path.splitext(os.path.basename(path))[0]
        v, f = _dev_mesh(mesh.read_obj(path), dev)
        m = (_unit_frame(v), f)
        (pts, nrm), = virtual_scan([m], poses, size=args.size, noise=args.noise, seed=args.seed)
        mesh.write_ply(os.path.join(args.out, name + '.ply'), pts, nrm)
        counts[name] = int(pts.shape[0])
        if args.normal_maps:
            maps = ray_images([m], poses, size=args.size, normalize=False)['normal'][0]
            for j in range(maps.shape[0]):
                render.write_png(os.path.join(args.out, 'view_%d' % j, name + '.png'), maps[j])
    res = {'shapes': len(files), 'views': len(poses), 'size': args.size, 'noise': args.noise, 'points': counts}
    print(json.dumps(res))
    return res


if __name__ == '__main__':
    main()
