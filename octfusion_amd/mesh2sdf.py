"""Triangle meshes to SDF lattices on the device (csrc/ofx_mesh2sdf.hip): the step before ``dataset.py``.

Replaces the reference's offline tools/repair_mesh.py::run_mesh2sdf (:122-156): load a raw ShapeNet OBJ, scale it into
[-0.8, 0.8]^3, ``mesh2sdf.compute(vertices, faces, 128, fix=True, level=0.015, return_mesh=True)`` -> a 128^3 SDF and a
repaired, watertight mesh; and sample_pts_from_mesh (:234-257 -> ``<name>/pointcloud.npz``).  ``prepare_mesh`` writes
exactly the files ``dataset.prepare_shape`` and ``dataset.ReadFile`` read next.

mesh2sdf itself is not available to compare against; include/ofx.h fixes the semantics and tests/mesh2sdf_oracle.py
restates them in float64.  Where this can differ from mesh2sdf:
  * the distance is the exact distance to the nearest triangle at EVERY lattice point; mesh2sdf computes it exactly in
    a band around the surface and sweeps it outwards (an approximation in the far field);
  * the sign is the parity of the crossings of the ray towards -x with a fixed tie rule (the rule of the level-set
    code mesh2sdf wraps, made exact), so an open or self-intersecting input gives the parity, not a heuristic;
  * the repair (fix=True) extracts the level set with the project's marching-cubes table (``mesh.marching_cubes``: the
    vertices of skimage's Lewiner tables, a different choice in ambiguous cells) and keeps the outer shell with
    ``mesh.largest_component``: components joined by shared vertices, the largest bounding-box side, where mesh2sdf
    walks its own connectivity.

    python -m octfusion_amd.mesh2sdf --input model.obj ... --out data [--size 128] [--level 0.015] [--pointcloud]
        [--no-fix] [--sign winding|auto [--beta B]] [--seed 0]
"""
import argparse
import os

import numpy as np
import torch

from . import _lib, mesh, mesh_check, mesh_query, metrics
from ._lib import call, ptr, stream

MESH_SCALE = 0.8           # tools/repair_mesh.py:127: the raw mesh is scaled into [-0.8, 0.8]^3
SHAPE_SCALE = 0.5          # tools/repair_mesh.py:36: the saved mesh and the dataset's points live in [-0.5, 0.5]^3
_INT32_MAX = 2 ** 31 - 1


def _device():
    return torch.device('cuda', torch.cuda.current_device())


def _max_batch(size):
    return max(1, _INT32_MAX // size ** 3)          # keeps the lattice of one call below 2^31 values


def mesh_to_sdf(meshes, size=128, signed=True, beta=0.0, stats=None):
    """SDF lattices [B, S, S, S] (fp32 on the device, x slowest) of ``meshes``, a list of B
    ``(verts [V, 3] fp32, faces [F, 3] int32)`` device tensors as ``mesh.marching_cubes`` returns them.  Lattice point
    ``(i, j, k)`` sits at ``2 (i, j, k) / S - 1`` -- what ``marching_cubes(sdf, level, bbmin=-1, bbmax=1)`` and
    ``dataset.py`` assume.  The magnitude is the exact distance to the nearest triangle (zero-area triangles count as
    the segment or point they are; vertices may lie outside the cube); with ``signed`` the value is negative where
    the ray towards -x crosses the surface an odd number of times, otherwise the distance is returned unsigned.
    ``signed='winding'``: the unsigned lattice, bit for bit, negated where the generalized winding number at the
    lattice point (``mesh_query.winding_number`` at its fp32 rounding, ``beta`` as there; exact by default) exceeds
    0.5 -- the sign for raw meshes that are open, self-intersecting or nested.  The lattice points are made on the
    device; further launches and host reads of status words only.
    ``signed='auto'``: per mesh, ray parity iff ``mesh_check.check`` (on the welded mesh) finds it watertight and free
    of self-intersections, else the winding number -- each lattice is, bit for bit, the one ``signed=True`` or
    ``signed='winding'`` gives that mesh.  ``stats`` (optional dict) receives ``sign``, the rule taken per mesh
    (``'parity'`` or ``'winding'``), and ``check``, the reports.
    Bitwise reproducible, and a shape's lattice does not depend on the batch it is in.

    One launch group (per ``(2^31 - 1) // S^3`` shapes) and one host read, the status words.  Raises ValueError naming
    the shape for a mesh without faces, a face index outside ``[0, V)`` or a non-finite vertex used by a face (nothing
    is read through a bad index), OfxError without a GPU (there is no CPU path)."""
    _lib.require_device()
    size = int(size)
    if not 2 <= size <= mesh.MAX_SIZE:
        raise ValueError('mesh_to_sdf: lattice size %d outside [2, %d]' % (size, mesh.MAX_SIZE))
    meshes = mesh._check_meshes(meshes, 'mesh_to_sdf')
    if not meshes:
        raise ValueError('mesh_to_sdf: no meshes')
    for k, (v, f) in enumerate(meshes):
        if f.shape[0] == 0 or v.shape[0] == 0:
            raise ValueError('mesh_to_sdf: shape %d has no faces' % k)
    if isinstance(signed, str) and signed == 'auto':
        return _sign_by_check(meshes, size, beta, stats)
    by_winding = mesh_query._winding_rule(signed, 'mesh_to_sdf')
    if stats is not None:
        stats['sign'] = ['winding' if by_winding else ('parity' if signed else 'none')] * len(meshes)
    out = []
    g = _max_batch(size)
    for b0 in range(0, len(meshes), g):
        out.append(_group(meshes[b0:b0 + g], b0, size, signed and not by_winding))
    sdf = out[0] if len(out) == 1 else torch.cat(out)
    return _sign_by_winding(meshes, sdf, size, beta) if by_winding else sdf


def _sign_by_check(meshes, size, beta, stats):
    """``signed='auto'``: the meshes ``mesh_check`` finds sound go through ray parity in one call, the others through
    the winding number in another (a shape's lattice does not depend on the batch it is in)."""
    reports = mesh_check.check(meshes)
    rule = ['parity' if mesh_check.ray_parity_is_sound(r) else 'winding' for r in reports]
    if stats is not None:
        stats['sign'] = rule
        stats['check'] = reports
    sdf = torch.empty(len(meshes), size, size, size, dtype=torch.float32, device=meshes[0][0].device)
    for name, signed in (('parity', True), ('winding', 'winding')):
        idx = [k for k, r in enumerate(rule) if r == name]
        if idx:
            sdf[idx] = mesh_to_sdf([meshes[k] for k in idx], size, signed=signed, beta=beta)
    return sdf


_WINDING_POINTS = 1 << 24          # lattice points of one winding call (192 MiB of queries)


def _sign_by_winding(meshes, sdf, S, beta):
    """Negates the unsigned lattices ``sdf [B, S, S, S]`` where the winding number at the lattice point exceeds 0.5.
    The points are made on the device, x-slabs of at most 2^24 points at a time for as many meshes as fit in that;
    per call one host read, the status words."""
    dev = sdf.device
    ax = ((2.0 * torch.arange(S, dtype=torch.float64, device=dev)) / S - 1.0).float()
    rows = max(1, _WINDING_POINTS // (S * S))                   # x-slabs per call
    flat = sdf.view(len(meshes), -1)
    for i0 in range(0, S, rows):
        i1 = min(S, i0 + rows)
        pts = torch.stack(torch.meshgrid(ax[i0:i1], ax, ax, indexing='ij'), dim=-1).reshape(-1, 3).contiguous()
        n = int(pts.shape[0])
        per = max(1, _WINDING_POINTS // n)
        for b0 in range(0, len(meshes), per):
            part = meshes[b0:b0 + per]
            inside = mesh_query.occupancy(part, [pts] * len(part), beta=beta)
            for k, occ in enumerate(inside):
                seg = flat[b0 + k, i0 * S * S:i1 * S * S]
                seg.copy_(torch.where(occ, -seg, seg))
    return sdf


def _group(part, b0, S, signed):
    B = len(part)
    dev = part[0][0].device
    verts, faces = mesh._cat(part)
    nv = [int(v.shape[0]) for v, _ in part]
    nf = [int(f.shape[0]) for _, f in part]
    if sum(nf) > _INT32_MAX:
        raise ValueError('mesh_to_sdf: more than 2^31 - 1 faces in one group')
    offs = torch.from_numpy(np.stack([np.concatenate([[0], np.cumsum(nv)]),
                                      np.concatenate([[0], np.cumsum(nf)])]).astype(np.int64)).to(dev)
    nbytes = _lib.lib().ofx_mesh_sdf_ws_bytes(B, sum(nv), sum(nf), S)
    if nbytes == 0:
        raise ValueError('mesh_to_sdf: %d shapes, %d vertices, %d faces out of range' % (B, sum(nv), sum(nf)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    sdf = torch.empty(B, S, S, S, dtype=torch.float32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    call('ofx_mesh_sdf', ptr(verts), ptr(faces), ptr(offs[0]), ptr(offs[1]), B, S, 1 if signed else 0, ptr(sdf),
         ptr(ws), ptr(status), stream())
    bad = torch.nonzero(status).flatten().tolist()              # the host read
    if bad:
        raise ValueError('mesh_to_sdf: shape %d has a face index outside [0, %d) or a non-finite vertex'
                         % (b0 + bad[0], nv[bad[0]]))
    return sdf


def _to_device_mesh(vertices, faces):
    _lib.require_device()
    dev = vertices.device if torch.is_tensor(vertices) and vertices.device.type == 'cuda' else _device()
    v = vertices if torch.is_tensor(vertices) else torch.from_numpy(np.ascontiguousarray(vertices, np.float32))
    f = faces if torch.is_tensor(faces) else torch.from_numpy(np.ascontiguousarray(faces, np.int64))
    return (v.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous(),
            f.to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous())


def compute(vertices, faces, size=128, fix=False, level=0.015, return_mesh=False, sign='parity', beta=0.0,
            stats=None):
    """mesh2sdf.compute with its argument order, so tools/repair_mesh.py:150 ports unchanged: ``vertices`` [V, 3] in
    [-1, 1]^3 and ``faces`` [F, 3] (numpy or tensors) -> the signed lattice [S, S, S] as a fp32 device tensor, and with
    ``return_mesh`` also the mesh ``(verts, faces)`` the lattice belongs to, as device tensors.

    fix=False: the signed lattice of the input as it is -- ``sign='parity'``: only meaningful for a watertight input;
      ``sign='winding'``: ``mesh_to_sdf(signed='winding', beta=beta)``, meaningful for a raw mesh too;
      ``sign='auto'``: ``mesh_to_sdf(signed='auto')`` -- parity iff ``mesh_check`` finds the input sound, else the
      winding number; ``stats`` (optional dict) receives the rule taken, as there.
    fix=True: the repair, composed from public calls only --
      1. ``u = mesh_to_sdf([input], size, signed=False)``, the unsigned distance;
      2. ``marching_cubes(u, level, bbmin=-1, bbmax=1)``: the surface at distance ``level`` around the input, an outer
         shell and, around closed parts, inner offset shells and cavities;
      3. ``largest_component``: the outer shell;
      4. ``mesh_to_sdf([shell], size, signed=True)``, returned with the shell.
    So the repaired surface lies ``level`` outside the input, as mesh2sdf's does.  See the module docstring for where
    the result can differ from mesh2sdf's (marching-cubes table, components by shared vertex, exact far field)."""
    if sign not in ('parity', 'winding', 'auto'):
        raise ValueError("compute: sign must be 'parity', 'winding' or 'auto', got %r" % (sign,))
    if fix and sign != 'parity':
        raise ValueError('compute: sign=%r needs fix=False (the repaired shell is watertight)' % (sign,))
    m = _to_device_mesh(vertices, faces)
    if not fix:
        sdf = mesh_to_sdf([m], size, signed=True if sign == 'parity' else sign, beta=beta, stats=stats)[0]
        return (sdf, m) if return_mesh else sdf
    u = mesh_to_sdf([m], size, signed=False)
    shell = mesh.largest_component(mesh.marching_cubes(u, float(level), bbmin=-1, bbmax=1))[0]
    if shell[1].shape[0] == 0:
        raise ValueError('compute: no surface at level %g on a lattice of %d' % (level, size))
    sdf = mesh_to_sdf([shell], size, signed=True)[0]
    return (sdf, shell) if return_mesh else sdf


def normalize(verts, mesh_scale=MESH_SCALE):
    """tools/repair_mesh.py:143-147: ``(verts', bbmin, bbmax)`` with ``verts' = (verts - centre) * 2 mesh_scale /
    largest bounding-box side``, in float64 numpy as the reference computes it."""
    v = verts.detach().cpu().numpy() if torch.is_tensor(verts) else np.asarray(verts)
    v = np.asarray(v, np.float64).reshape(-1, 3)
    if len(v) == 0:
        raise ValueError('normalize: no vertices')
    bbmin, bbmax = v.min(0), v.max(0)
    center = (bbmin + bbmax) * 0.5
    extent = (bbmax - bbmin).max()
    if not extent > 0:
        raise ValueError('normalize: the mesh has no extent')
    scale = 2.0 * mesh_scale / extent
    return (v - center) * scale, bbmin, bbmax


def read_mesh(path):
    """(verts [V, 3] float32, faces [F, 3] int32, 0-based) of an OBJ as raw ShapeNet files are written: ``v`` lines;
    ``f`` lines with ``v``, ``v/vt``, ``v//vn`` or ``v/vt/vn`` tokens, positive (1-based) or negative (relative to the
    vertices read so far) indices, and polygons of any size, which are fan-triangulated around their first vertex.
    Everything else (normals, texture coordinates, groups, materials) is ignored."""
    vs, fs = [], []
    with open(path) as fh:
        for line in fh:
            t = line.split()
            if not t:
                continue
            if t[0] == 'v':
                vs.append(t[1:4])
            elif t[0] == 'f':
                idx = []
                for tok in t[1:]:
                    i = int(tok.split('/')[0])
                    idx.append(i - 1 if i > 0 else len(vs) + i)
                for k in range(1, len(idx) - 1):
                    fs.append((idx[0], idx[k], idx[k + 1]))
    v = np.asarray(vs, np.float64).astype(np.float32).reshape(-1, 3)
    f = np.asarray(fs, np.int64).astype(np.int32).reshape(-1, 3)
    return v, f


def prepare_mesh(path, name, sdf_dir, mesh_dir, bbox_dir, dataset_dir=None, size=128, level=0.015, points=100000,
                 seed=0, fix=True, sign='parity', beta=0.0):
    """run_mesh2sdf (tools/repair_mesh.py:139-156) for one raw mesh, plus sample_pts_from_mesh (:250-257) with
    ``dataset_dir``: read ``path``, ``normalize`` it, ``compute(fix=True, return_mesh=True)`` and write
      ``sdf_dir/<name>.npy``    the lattice [S, S, S] fp32,
      ``mesh_dir/<name>.obj``   the repaired mesh, vertices * 0.5 (shape_scale),
      ``bbox_dir/<name>.npz``   bbmax, bbmin (of the raw vertices, float64) and mul = 0.8,
      ``dataset_dir/<name>/pointcloud.npz``  ``points`` [n, 3] and ``normals`` [n, 3] fp16 drawn from the saved mesh by
                                ``metrics.sample_surface(normals=True, normalize=False)`` (seeded: reproducible).
    Returns the list of files written.  fix=False skips the repair (a mesh known to be watertight); with
    ``sign='winding'`` it writes the signed lattice of the raw mesh itself, signed by its winding number."""
    v, f = read_mesh(path)
    if len(f) == 0:
        raise ValueError('prepare_mesh: %s has no faces' % path)
    vn, bbmin, bbmax = normalize(v, MESH_SCALE)
    sdf, (mv, mf) = compute(vn, f, size, fix=fix, level=level, return_mesh=True, sign=sign, beta=beta)
    mv = mv * SHAPE_SCALE
    files = [os.path.join(sdf_dir, name + '.npy'), os.path.join(mesh_dir, name + '.obj'),
             os.path.join(bbox_dir, name + '.npz')]
    for p in files:
        os.makedirs(os.path.dirname(p), exist_ok=True)
    np.save(files[0], sdf.cpu().numpy())
    mesh.write_obj(files[1], mv, mf)
    np.savez(files[2], bbmax=bbmax, bbmin=bbmin, mul=MESH_SCALE)
    if dataset_dir is not None:
        from .dataset import shape_id
        pts, nrm = metrics.sample_surface([(mv, mf)], int(points), seed, normalize=False, ids=[shape_id(name)],
                                          normals=True)
        out = os.path.join(dataset_dir, name, 'pointcloud.npz')
        os.makedirs(os.path.dirname(out), exist_ok=True)
        np.savez(out, points=pts[0].cpu().numpy().astype(np.float16), normals=nrm[0].cpu().numpy().astype(np.float16))
        files.append(out)
    return files


# ---------------------------------------------------------------------------------------------------- driver
def shape_name(path):
    """ShapeNet keeps ``<category>/<id>/model.obj``: the name is ``<category>/<id>``; any other file is named by its
    base name."""
    path = os.path.normpath(path)
    stem = os.path.splitext(os.path.basename(path))[0]
    if stem == 'model':
        parts = os.path.dirname(path).split(os.sep)
        return '/'.join(p for p in parts[-2:] if p) or stem
    return stem


def parser():
    ap = argparse.ArgumentParser(prog='python -m octfusion_amd.mesh2sdf', description=__doc__.split('\n\n')[0])
    ap.add_argument('--input', required=True, nargs='+', metavar='PATH', help='OBJ files (polygons, v/vt/vn tokens '
                    'and negative indices are understood)')
    ap.add_argument('--out', required=True, metavar='ROOT', help='receives sdf/<name>.npy, mesh/<name>.obj, '
                    'bbox/<name>.npz and, with --pointcloud, dataset/<name>/pointcloud.npz')
    ap.add_argument('--size', type=int, default=128, help='lattice size S')
    ap.add_argument('--level', type=float, default=0.015, help='offset of the repaired surface (2 / S is one cell)')
    ap.add_argument('--pointcloud', action='store_true', help='also draw the oriented point cloud of the saved mesh')
    ap.add_argument('--points', type=int, default=100000, help='points of the cloud')
    ap.add_argument('--no-fix', action='store_true', help='the input is watertight: take its signed lattice as it is')
    ap.add_argument('--sign', choices=['parity', 'winding', 'auto'], default='parity', help="'winding': the signed "
                    "lattice of the raw mesh itself, signed by its winding number; 'auto': by parity if mesh_check "
                    'finds the mesh watertight and free of self-intersections, else by the winding number (both imply '
                    '--no-fix)')
    ap.add_argument('--beta', type=float, default=mesh_query.DEFAULT_CLI_BETA, help='far-field opening of --sign '
                    'winding / auto (0: exact)')
    ap.add_argument('--seed', type=int, default=0)
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    _lib.require_device()
    root = args.out
    for path in args.input:
        prepare_mesh(path, shape_name(path), os.path.join(root, 'sdf'), os.path.join(root, 'mesh'),
                     os.path.join(root, 'bbox'), os.path.join(root, 'dataset') if args.pointcloud else None,
                     args.size, args.level, args.points, args.seed, fix=not (args.no_fix or args.sign != 'parity'),
                     sign=args.sign, beta=args.beta if args.sign != 'parity' else 0.0)
    print('mesh2sdf: %d shapes written under %s' % (len(args.input), root))


if __name__ == '__main__':
    main()
