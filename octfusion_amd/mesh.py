"""Mesh export of the generate path: marching cubes on the device (csrc/ofx_mesh.hip), an OBJ writer and a PLY
point-cloud writer.

Replaces the reference's host tail (export_mesh, models/octfusion_model_union.py:435-468; create_mesh,
utils/util_dualoctree.py:120-142): skimage.measure.marching_cubes(sdf, level=0) per shape, vertices mapped by
``vtx * ((bbmax - bbmin) / size) + bbmin`` and ``* point_scale``, written as ``<index>.obj`` by trimesh.

Differences from the reference:
  * the triangulation table is the project's own (tools/gen_mc_table.py): same vertices as skimage (one per crossing
    lattice edge, linear interpolation), but in ambiguous cells the topology may differ from the Lewiner tables;
  * an empty shape is skipped with a warning -- the reference returns at the first empty shape and drops the rest of
    the batch (octfusion_model_union.py:453-455);
  * clean=True (keep the component whose bounding box has the largest side, :459-467) runs on the device
    (csrc/ofx_mesh_cc.hip: components, largest_component): connectivity is by shared vertex where trimesh uses edges
    shared by exactly two faces, extents are fp32, a tie goes to the lowest vertex id.
"""
import ctypes
import os
import warnings

import numpy as np
import torch

from . import _lib

# point_scale of each diffusion config's VAE eval YAML (reference configs/vae_snet_eval.yaml:52,86: 0.5;
# configs/vae_obja_eval_depth864.yaml:52,86: 1.0): export_mesh multiplies the vertices by it
# (octfusion_model_union.py:442,457).  Kept here rather than in configs.py, whose dicts are U-Net constructor kwargs
# and whose bytes key the committed oracle fixtures.
MESH_SCALES = {'snet_uncond': 0.5, 'snet_cond': 0.5, 'obja_uncond': 1.0}

MAX_SIZE = 512          # csrc/ofx_mesh.hip: the id map packs a 29-bit vertex id
MAX_TRI_PER_CELL = 5    # every count of one call goes through one int32 scan (include/ofx.h)
MAX_BATCH = 65535       # shapes per call of the library (include/ofx.h: a grid dimension of the count pass)


def mesh_scale(config):
    """The reference's point_scale for a config name of octfusion_amd.configs."""
    return MESH_SCALES[config]


def _max_batch(size):
    return min(MAX_BATCH, max(1, (2 ** 31 - 1) // (MAX_TRI_PER_CELL * size ** 3)))


def marching_cubes(sdfs, level=0.0, bbmin=-0.9, bbmax=0.9, scale=1.0, clean=False, stats=None):
    """Meshes of a batch of SDF lattices ``sdfs`` [B, R, R, R] (fp32 on the device, x slowest; what
    ``mpu.calc_sdf`` and the pipeline produce).  Returns a list of B ``(verts [V, 3] fp32, faces [F, 3] int32)``
    device tensors: vertices in ``(index * (bbmax - bbmin) / R + bbmin) * scale`` coordinates, faces 0-based into
    that shape's own vertices, wound so that the normals point to increasing values (outward for an SDF that is
    negative inside).

    Makes ONE host synchronisation: the per-shape counts are read back between the count and the emit pass (once
    per group of ``min(65535, (2^31 - 1) // (5 R^3))`` shapes -- 25 at R = 256).  Raises ValueError naming the shape if a cell
    of it has a non-finite corner, and OfxError without a GPU (there is no CPU path).

    clean=True keeps only each shape's largest component (the reference's export_mesh clean=True; what
    ``largest_component`` returns), straight from the batch buffers the mesher wrote, for one more host
    synchronisation per group (the kept counts).  stats (optional dict, with clean): ``stats['components']`` becomes
    the list of the shapes' component counts before cleaning."""
    _lib.require_device()
    if sdfs.dim() != 4 or not (sdfs.shape[1] == sdfs.shape[2] == sdfs.shape[3]):
        raise ValueError('marching_cubes: sdfs must be [B, R, R, R], got %s' % (tuple(sdfs.shape),))
    B, R = int(sdfs.shape[0]), int(sdfs.shape[1])
    if not 2 <= R <= MAX_SIZE:
        raise ValueError('marching_cubes: lattice size %d outside [2, %d]' % (R, MAX_SIZE))
    if not np.isfinite(level):
        raise ValueError('marching_cubes: level must be finite')
    if sdfs.device.type != 'cuda' or sdfs.dtype != torch.float32:
        raise ValueError('marching_cubes: sdfs must be a float32 device tensor')
    sdfs = sdfs.contiguous()
    step = (float(bbmax) - float(bbmin)) / R
    out = []
    comps = [] if clean else None
    g = _max_batch(R)
    for b0 in range(0, B, g):
        out += _group(sdfs[b0:b0 + g], b0, R, float(level), step, float(bbmin), float(scale), comps)
    if clean and stats is not None:
        stats['components'] = comps
    return out


def _group(sdf, b0, R, level, step, bbmin, scale, comps=None):
    B = int(sdf.shape[0])
    dev = sdf.device
    st = _lib.stream()
    ws = torch.empty(_lib.lib().ofx_mc_ws_bytes(B, R), dtype=torch.uint8, device=dev)
    counts = torch.empty(B * 3, dtype=torch.int64, device=dev)
    _lib.call('ofx_mc_count', _lib.ptr(sdf), B, R, level, _lib.ptr(ws), _lib.ptr(counts), st)
    c = counts.view(B, 3).cpu()                        # the host sync
    bad = torch.nonzero(c[:, 2]).flatten().tolist()
    if bad:
        raise ValueError('marching_cubes: shape %d has %d cells with a non-finite corner'
                         % (b0 + bad[0], int(c[bad[0], 2])))
    nv, nt = c[:, 0], c[:, 1]
    voff = torch.cumsum(nv, 0) - nv
    toff = torch.cumsum(nt, 0) - nt
    V, T = int(nv.sum()), int(nt.sum())
    verts = torch.empty(max(V, 1), 3, dtype=torch.float32, device=dev)
    faces = torch.empty(max(T, 1), 3, dtype=torch.int32, device=dev)
    offs = torch.stack([voff, toff]).to(dev)
    _lib.call('ofx_mc_emit', _lib.ptr(sdf), B, R, level, step, bbmin, scale, _lib.ptr(ws), _lib.ptr(offs[0]),
              _lib.ptr(offs[1]), _lib.ptr(verts), _lib.ptr(faces), st)
    if comps is not None:                              # clean=True: the batch buffers go on as they are
        return _clean(verts, faces, nv.tolist(), nt.tolist(), comps)
    return [(verts[int(voff[b]):int(voff[b] + nv[b])], faces[int(toff[b]):int(toff[b] + nt[b])]) for b in range(B)]


# ---- field meshing (csrc/ofx_fieldmesh.hip): marching cubes without the dense lattice --------------------------------
FIELD_MAX_SIZE = 2048
FIELD_MAX_BATCH = 128                          # shapes per call of the library
FIELD_GROUP_BRICKS = 1 << 22                   # active bricks a call aims at (18 GB of workspace); one shape may pass
FIELD_MAX_COUNT = 2 ** 31 - 1                  # vertices, and triangles, of one call: its emit pass scans them in int32
FIELD_BRICK_BYTES = 4404                       # workspace per active brick: 729 samples, 16-bit id map, counts, scans


def field_mesh(field, size, level=0.0, bbmin=-0.9, bbmax=0.9, scale=1.0, margin=1, clean=False, stats=None,
               shapes=None):
    """Meshes of the decoded NeuralMPU ``field`` (an ``mpu.MpuField``) on the ``size``^3 lattice of ``mpu.calc_sdf``,
    2 <= size <= 2048, without ever holding that lattice: the field is evaluated only in bricks of 8^3 cells within
    ``margin`` finest-level octree cells of a node at ``field.depth_out`` and meshed from there.  Returns what
    ``marching_cubes(calc_sdf(field, ...))`` returns -- a list of ``(verts [V, 3] fp32, faces [F, 3] int32)`` device
    tensors, one per shape, same coordinates, table and winding -- restricted to the cells of the active bricks;
    sample values are bit-equal to the sweep's.  A surface sheet the field produces inside a coarse leaf, farther than
    the margin from every finest node, is NOT meshed (the dense path finds it); ``leaks`` tells whether the surface
    reached the edge of the band.  Vertices are ordered by (brick, point in the brick, axis), triangles by (brick, cell,
    table order); the output is bitwise reproducible and a shape's mesh does not depend on the rest of the batch.

    shapes: the batch indices to mesh (default: all), in the order of the result.  clean=True keeps each shape's
    largest component.  stats (optional dict) gains ``seeds`` (bricks active at margin 0), ``bricks`` (active bricks),
    ``leaks`` (crossing lattice edges on a face between an active and an inactive brick) and ``total_bricks`` (bricks
    of the lattice), lists with one entry per meshed shape, and ``components`` with clean.

    Two host synchronisations per group of shapes (the brick counts, then the vertex / triangle counts); device
    memory is 4404 B per active brick plus the nb^3 brick flags and the output.  A shape is never cut: whatever number
    of its bricks is active, up to all 2^24 of a 2048^3 lattice, goes through one call.  A batch is cut into groups of
    consecutive shapes of about 4 M active bricks, and again if a group's vertices or triangles would pass 2^31 - 1.
    Raises ValueError for a bad argument, for a shape whose active cells have a non-finite corner, and for a single
    shape with more than 2^31 - 1 vertices or triangles (its faces are int32); OfxError without a GPU."""
    from . import mpu
    _lib.require_device()
    if not isinstance(field, mpu.MpuField):
        raise ValueError('field_mesh: field must be an mpu.MpuField')
    size, margin = int(size), int(margin)
    if not 2 <= size <= FIELD_MAX_SIZE:
        raise ValueError('field_mesh: lattice size %d outside [2, %d]' % (size, FIELD_MAX_SIZE))
    if not np.isfinite(level):
        raise ValueError('field_mesh: level must be finite')
    if margin < 0:
        raise ValueError('field_mesh: margin must be >= 0')
    if not (np.isfinite(bbmin) and np.isfinite(bbmax) and np.isfinite(scale) and bbmax > bbmin):
        raise ValueError('field_mesh: needs finite bbmin < bbmax and a finite scale')
    octree = field.octree
    if not 0 <= field.full_depth <= field.depth_out <= octree.depth:
        raise ValueError('field_mesh: depth_out %d outside [full_depth %d, octree depth %d]'
                         % (field.depth_out, field.full_depth, octree.depth))
    B = int(octree.batch_size)
    shapes = list(range(B)) if shapes is None else [int(b) for b in shapes]
    if any(not 0 <= b < B for b in shapes):
        raise ValueError('field_mesh: shapes must lie in [0, %d)' % B)
    h = mpu._TreeHandle.of(octree)
    code = mpu._code(field.reg, h, field.full_depth, field.depth_out)
    geo = (size, float(level), (float(bbmax) - float(bbmin)) / size, float(bbmin), float(scale), margin)
    runs = []                                              # consecutive batch indices: one library call each
    for b in shapes:
        if runs and runs[-1][-1] + 1 == b and len(runs[-1]) < FIELD_MAX_BATCH:
            runs[-1].append(b)
        else:
            runs.append([b])
    out, acc = [], dict(seeds=[], bricks=[], leaks=[], components=[] if clean else None)
    for run in runs:
        out += _field_run(field, h, code, run[0], len(run), geo, acc)
    if stats is not None:
        stats.update(seeds=acc['seeds'], bricks=acc['bricks'], leaks=acc['leaks'],
                     total_bricks=[(-(-(size - 1) // 8)) ** 3] * len(shapes))
        if clean:
            stats['components'] = acc['components']
    return out


def _field_classify(field, h, code, b0, B, geo):
    """(classify workspace, [B, 2] host tensor of active bricks and seeds) of shapes b0 .. b0 + B - 1: host sync 1."""
    size, level, step, bbmin, scale, margin = geo
    cws = torch.empty(_lib.lib().ofx_fieldmesh_classify_ws_bytes(B, size), dtype=torch.uint8, device=code.device)
    bc = torch.empty(B * 2, dtype=torch.int64, device=code.device)
    _lib.call('ofx_fieldmesh_classify', ctypes.byref(h.tree), field.depth_out, b0, B, size, step, bbmin, margin,
              _lib.ptr(cws), _lib.ptr(bc), _lib.stream())
    return cws, bc.view(B, 2).cpu()


def _field_run(field, h, code, b0, B, geo, acc):
    """Consecutive shapes b0 .. b0 + B - 1: one group if their active bricks fit FIELD_GROUP_BRICKS, else groups of
    consecutive shapes that do (a shape on its own may be larger), each classified once more on its own -- the ranks
    a classify workspace holds are those of the shapes it was called for."""
    cws, bc = _field_classify(field, h, code, b0, B, geo)
    nb = bc[:, 0].tolist()
    if B == 1 or sum(nb) <= FIELD_GROUP_BRICKS:
        return _field_group(field, h, code, b0, B, geo, acc, cws, bc)
    del cws
    parts, cur = [[0, 0]], 0
    for k in range(B):
        if parts[-1][1] and cur + nb[k] > FIELD_GROUP_BRICKS:
            parts.append([k, 0])
            cur = 0
        parts[-1][1] += 1
        cur += nb[k]
    out = []
    for k, cnt in parts:
        out += _field_group(field, h, code, b0 + k, cnt, geo, acc, *_field_classify(field, h, code, b0 + k, cnt, geo))
    return out


def _field_group(field, h, code, b0, B, geo, acc, cws, bc):
    size, level, step, bbmin, scale, margin = geo
    dev = code.device
    st = _lib.stream()
    L = _lib.lib()
    tree = ctypes.byref(h.tree)
    n = int(bc[:, 0].sum())
    empty = (torch.empty(0, 3, dtype=torch.float32, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev))
    if n == 0:
        acc['bricks'] += bc[:, 0].tolist()
        acc['seeds'] += bc[:, 1].tolist()
        acc['leaks'] += [0] * B
        if acc['components'] is not None:
            acc['components'] += [0] * B
        return [empty for _ in range(B)]
    ws = torch.empty(L.ofx_fieldmesh_ws_bytes(n), dtype=torch.uint8, device=dev)
    counts = torch.empty(B * 4, dtype=torch.int64, device=dev)
    _lib.call('ofx_fieldmesh_count', tree, field.full_depth, field.depth_out, _lib.ptr(code), b0, B, size, step, bbmin,
              level, _lib.ptr(cws), n, _lib.ptr(ws), _lib.ptr(counts), st)
    c = counts.view(B, 4).cpu()                        # host sync 2
    bad = torch.nonzero(c[:, 2]).flatten().tolist()
    if bad:
        raise ValueError('field_mesh: shape %d has %d cells with a non-finite corner'
                         % (b0 + bad[0], int(c[bad[0], 2])))
    nv, nt = c[:, 0], c[:, 1]
    if max(int(nv.sum()), int(nt.sum())) > FIELD_MAX_COUNT:    # the emit pass scans a call's counts in int32
        if B == 1:
            raise ValueError('field_mesh: shape %d has %d vertices and %d triangles, more than %d'
                             % (b0, int(nv[0]), int(nt[0]), FIELD_MAX_COUNT))
        del ws, cws
        out = []
        for k, cnt in ((0, B // 2), (B // 2, B - B // 2)):
            out += _field_group(field, h, code, b0 + k, cnt, geo, acc,
                                *_field_classify(field, h, code, b0 + k, cnt, geo))
        return out
    acc['bricks'] += bc[:, 0].tolist()
    acc['seeds'] += bc[:, 1].tolist()
    acc['leaks'] += c[:, 3].tolist()
    voff = torch.cumsum(nv, 0) - nv
    toff = torch.cumsum(nt, 0) - nt
    V, T = int(nv.sum()), int(nt.sum())
    verts = torch.empty(max(V, 1), 3, dtype=torch.float32, device=dev)
    faces = torch.empty(max(T, 1), 3, dtype=torch.int32, device=dev)
    offs = torch.stack([voff, toff]).to(dev)
    _lib.call('ofx_fieldmesh_emit', B, size, level, step, bbmin, scale, _lib.ptr(cws), n, _lib.ptr(ws),
              _lib.ptr(offs[0]), _lib.ptr(offs[1]), _lib.ptr(verts), _lib.ptr(faces), st)
    if acc['components'] is not None:
        return _clean(verts, faces, nv.tolist(), nt.tolist(), acc['components'])
    return [(verts[int(voff[b]):int(voff[b] + nv[b])], faces[int(toff[b]):int(toff[b] + nt[b])]) for b in range(B)]


# ---- components (csrc/ofx_mesh_cc.hip): export_mesh's clean=True, octfusion_model_union.py:459-467 ------------------
_INT32_MAX = 2 ** 31 - 1
_last_cc_status = (0, 0)


def last_cc_status():
    """(loop cap tripped, bad face index) words of the latest component call, as read back with its counts."""
    return _last_cc_status


def _check_meshes(meshes, who):
    meshes = list(meshes)
    for k, m in enumerate(meshes):
        if not (isinstance(m, (tuple, list)) and len(m) == 2 and torch.is_tensor(m[0]) and torch.is_tensor(m[1])):
            raise ValueError('%s: shape %d is not a (verts, faces) pair of tensors' % (who, k))
        v, f = m
        if v.device.type != 'cuda' or f.device.type != 'cuda' or v.device != f.device:
            raise ValueError('%s: shape %d is not on the device' % (who, k))
        if v.dtype != torch.float32 or f.dtype != torch.int32:
            raise ValueError('%s: shape %d must have float32 vertices and int32 faces' % (who, k))
        if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
            raise ValueError('%s: shape %d must be verts [V, 3], faces [F, 3]' % (who, k))
        if v.shape[0] > _INT32_MAX or f.shape[0] > _INT32_MAX:
            raise ValueError('%s: shape %d has more than 2^31 - 1 vertices or faces' % (who, k))
    return meshes


def _mesh_groups(meshes):
    """Runs of consecutive meshes whose vertices and whose faces each fit one int32 scan (as _max_batch does)."""
    groups, cur, V, F = [], [], 0, 0
    for k, (v, f) in enumerate(meshes):
        if cur and (V + v.shape[0] > _INT32_MAX or F + f.shape[0] > _INT32_MAX):
            groups.append(cur)
            cur, V, F = [], 0, 0
        cur.append(k)
        V += int(v.shape[0])
        F += int(f.shape[0])
    if cur:
        groups.append(cur)
    return groups


def _cat(meshes):
    if len(meshes) == 1:
        return meshes[0][0].contiguous(), meshes[0][1].contiguous()
    return torch.cat([v for v, _ in meshes]).contiguous(), torch.cat([f for _, f in meshes]).contiguous()


# ---- the triangle bins (csrc/ofx_tribins.hip): what the callers of ofx_mesh_query and ofx_ray_cast share -----------
MAX_BINS = 16
_MAX_Q = 2 ** 30


def _gather(meshes, sets, bins, who, noun):
    """The argument checks and the concatenated arrays of one call that searches the bins of ``meshes``.

    sets: ``(what, label, value)`` per kind of per-mesh ``[n, 3]`` fp32 set -- ``what`` names one set and keys the
    result, ``label`` names the list (``('points', 'point sets', points)``); value is a list of B tensors or one
    ``[B, n, 3]`` tensor.  Every kind has the same count per mesh.  who, noun: the caller and what it counts
    (``'queries'``), for the messages.  Returns a dict: verts, faces, one concatenated tensor per ``what``, offs
    ``[3, B + 1]`` int64 on the device (vertices, faces, items), the host lists nv, nf, nq, and B, bins, dev."""
    bins = int(bins)
    if not 0 <= bins <= MAX_BINS:
        raise ValueError('%s: bins %d outside [0, %d]' % (who, bins, MAX_BINS))
    meshes = _check_meshes(meshes, who)
    if not meshes:
        raise ValueError('%s: no meshes' % who)
    B, dev = len(meshes), meshes[0][0].device
    for k, (v, f) in enumerate(meshes):
        if f.shape[0] == 0 or v.shape[0] == 0:
            raise ValueError('%s: shape %d has no faces' % (who, k))
        if v.device != dev:
            raise ValueError('%s: shape %d is on another device' % (who, k))
    lists = []
    for what, label, value in sets:
        if torch.is_tensor(value) and (value.dim() != 3 or value.shape[2] != 3):
            raise ValueError('%s: a stacked batch of %s must be [B, n, 3], got %s' % (who, what, tuple(value.shape)))
        value = list(value)
        if len(value) != B:
            raise ValueError('%s: %d %s for %d meshes' % (who, len(value), label, B))
        for k, p in enumerate(value):
            if not torch.is_tensor(p) or p.dim() != 2 or p.shape[1] != 3:
                raise ValueError('%s: %s %d must be a [n, 3] tensor' % (who, what, k))
            if p.dtype != torch.float32:
                raise ValueError('%s: %s %d must be float32, got %s' % (who, what, k, p.dtype))
            if p.device != dev:
                raise ValueError('%s: %s %d are not on the device of the meshes' % (who, what, k))
            if lists and p.shape[0] != lists[0][k].shape[0]:
                raise ValueError('%s: %d %s for %d %s of shape %d'
                                 % (who, lists[0][k].shape[0], sets[0][0], p.shape[0], what, k))
        lists.append(value)
    nv = [int(v.shape[0]) for v, _ in meshes]
    nf = [int(f.shape[0]) for _, f in meshes]
    nq = [int(p.shape[0]) for p in lists[0]]
    if sum(nf) > _INT32_MAX or sum(nq) > _MAX_Q or B > 65535:
        raise ValueError('%s: %d shapes, %d faces, %d %s exceed one call (65535, 2^31 - 1, 2^30)'
                         % (who, B, sum(nf), sum(nq), noun))
    verts, faces = _cat(meshes)
    offs = torch.from_numpy(np.stack([np.cumsum([0] + nv), np.cumsum([0] + nf),
                                      np.cumsum([0] + nq)]).astype(np.int64)).to(dev)
    g = dict(verts=verts, faces=faces, offs=offs, nv=nv, nf=nf, nq=nq, B=B, bins=bins, dev=dev)
    for (what, _, _), value in zip(sets, lists):
        g[what] = value[0].contiguous() if B == 1 else torch.cat(value).contiguous()
    return g


def _bins_ws(g, ws_bytes, who, noun):
    """The workspace of a gathered call, sized by the library's ``ws_bytes`` entry (its name)."""
    sizes = (g['B'], sum(g['nv']), sum(g['nf']), sum(g['nq']))
    nbytes = getattr(_lib.lib(), ws_bytes)(*sizes, g['bins'])
    if nbytes == 0:
        raise ValueError('%s: %d shapes, %d vertices, %d faces, %d %s out of range' % ((who,) + sizes + (noun,)))
    return torch.empty(nbytes, dtype=torch.uint8, device=g['dev'])


def _raise_bad_shape(status, g, who):
    """Reads the status words of a gathered call (a host read) and refuses the first shape the device refused."""
    bad = torch.nonzero(status).flatten().tolist()
    if bad:
        raise ValueError('%s: shape %d has a face index outside [0, %d) or a non-finite vertex'
                         % (who, bad[0], g['nv'][bad[0]]))


def _label(verts, faces, nv, nf):
    """Label one batch mesh: (offsets [2, B + 1] on the device, label, workspace, status words)."""
    B, V, F = len(nv), sum(nv), sum(nf)
    dev = faces.device
    nbytes = _lib.lib().ofx_mesh_cc_ws_bytes(V, F, B)
    if nbytes == 0:
        raise ValueError('mesh components: %d vertices, %d faces outside [1, 2^31 - 1]' % (V, F))
    offs = torch.from_numpy(np.stack([np.concatenate([[0], np.cumsum(nv)]),
                                      np.concatenate([[0], np.cumsum(nf)])]).astype(np.int64)).to(dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    label = torch.empty(V, dtype=torch.int32, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.call('ofx_mesh_cc_label', _lib.ptr(faces), _lib.ptr(offs[0]), _lib.ptr(offs[1]), B, V, F, _lib.ptr(label),
              _lib.ptr(ws), _lib.ptr(status), _lib.stream())
    return offs, label, ws, status


def _read_back(counts, status, who):
    """The one host synchronisation of a pass: its counts and the two status words."""
    global _last_cc_status
    host = torch.cat([counts.flatten().to(torch.int64), status.to(torch.int64)]).cpu()
    cap, bad = int(host[-2]), int(host[-1])
    _last_cc_status = (cap, bad)
    if bad:
        raise ValueError('%s: %s' % (who, 'a face index lies outside [0, V) of its shape' if bad & 1
                                     else 'inconsistent offsets'))
    if cap:
        raise _lib.OfxError('%s: a union-find loop hit its cap (status %d)' % (who, cap))
    return host[:-2]


def _clean(verts, faces, nv, nf, comps=None, who='largest_component'):
    """Largest component of every shape of one batch mesh (nv / nf: per-shape counts on the host)."""
    B, V, F = len(nv), sum(nv), sum(nf)
    if F == 0 or V == 0:
        if comps is not None:
            comps += [0] * B
        return [(verts[:0], faces[:0]) for _ in range(B)]
    dev = faces.device
    st = _lib.stream()
    offs, label, ws, status = _label(verts, faces, nv, nf)
    winner = torch.empty(B, dtype=torch.int32, device=dev)
    keep = torch.empty(3 * B, dtype=torch.int64, device=dev)
    _lib.call('ofx_mesh_cc_select', _lib.ptr(verts), _lib.ptr(faces), _lib.ptr(label), _lib.ptr(offs[0]),
              _lib.ptr(offs[1]), B, V, F, _lib.ptr(winner), _lib.ptr(keep), _lib.ptr(ws), _lib.ptr(status), st)
    c = _read_back(keep, status, who).view(3, B)       # the host sync
    kv, kf = c[0], c[1]
    if comps is not None:
        comps += c[2].tolist()
    nvo = torch.cumsum(kv, 0) - kv
    nfo = torch.cumsum(kf, 0) - kf
    out_v = torch.empty(max(int(kv.sum()), 1), 3, dtype=torch.float32, device=dev)
    out_f = torch.empty(max(int(kf.sum()), 1), 3, dtype=torch.int32, device=dev)
    new = torch.stack([nvo, nfo]).to(dev)
    _lib.call('ofx_mesh_cc_extract', _lib.ptr(verts), _lib.ptr(faces), _lib.ptr(offs[0]), _lib.ptr(offs[1]), B, V, F,
              _lib.ptr(new[0]), _lib.ptr(new[1]), _lib.ptr(out_v), _lib.ptr(out_f), _lib.ptr(ws), _lib.ptr(status), st)
    return [(out_v[int(nvo[b]):int(nvo[b] + kv[b])], out_f[int(nfo[b]):int(nfo[b] + kf[b])]) for b in range(B)]


def largest_component(meshes, stats=None):
    """The reference's ``export_mesh(clean=True)`` rule (octfusion_model_union.py:459-467) on the device: of every
    mesh of ``meshes`` -- ``(verts [V, 3] fp32, faces [F, 3] int32)`` device tensors, as ``marching_cubes`` returns
    them -- keep the connected component whose bounding box has the largest side.  Two vertices are connected when
    a face uses both; a tie goes to the component with the lowest vertex id.  Returns a list of pairs of the same
    types: kept vertices and faces in their original order, indices renumbered, bitwise reproducible.  A mesh with
    one component comes back with equal contents (minus vertices no face uses); a mesh without faces comes back
    empty.  One host synchronisation per group (the kept counts).  stats (optional dict): ``stats['components']``
    becomes the component counts before cleaning.  Raises ValueError for a wrong dtype or device or a face index
    outside ``[0, V)`` (checked on the device before anything follows an index), OfxError without a GPU."""
    _lib.require_device()
    meshes = _check_meshes(meshes, 'largest_component')
    out, comps = [], []
    for grp in _mesh_groups(meshes):
        part = [meshes[k] for k in grp]
        v, f = _cat(part)
        out += _clean(v, f, [int(m[0].shape[0]) for m in part], [int(m[1].shape[0]) for m in part], comps)
    if stats is not None:
        stats['components'] = comps
    return out


def components(meshes):
    """The component table of every mesh of ``meshes`` (device ``(verts, faces)`` pairs as for
    ``largest_component``): one dict per shape with ``comp_of_vert`` int32 [V] (-1 for a vertex no face uses),
    ``comp_of_face`` int32 [F], ``bbox_min`` / ``bbox_max`` fp32 [K, 3] (exact minima / maxima of the stored
    coordinates) and ``n_verts`` / ``n_faces`` int64 [K].  Components are numbered by their lowest vertex id; only
    components with a face are listed (an empty mesh: K = 0).  One host synchronisation per group (the component
    counts).  Same errors as ``largest_component``."""
    _lib.require_device()
    meshes = _check_meshes(meshes, 'components')
    out = []
    for grp in _mesh_groups(meshes):
        part = [meshes[k] for k in grp]
        nv = [int(m[0].shape[0]) for m in part]
        nf = [int(m[1].shape[0]) for m in part]
        out += _components(*_cat(part), nv, nf)
    return out


def _components(verts, faces, nv, nf):
    B, V, F = len(nv), sum(nv), sum(nf)
    dev = faces.device
    if F == 0 or V == 0:
        return [dict(comp_of_vert=torch.full((n,), -1, dtype=torch.int32, device=dev),
                     comp_of_face=torch.empty(0, dtype=torch.int32, device=dev),
                     bbox_min=torch.empty(0, 3, device=dev), bbox_max=torch.empty(0, 3, device=dev),
                     n_verts=torch.empty(0, dtype=torch.int64, device=dev),
                     n_faces=torch.empty(0, dtype=torch.int64, device=dev)) for n in nv]
    st = _lib.stream()
    offs, label, ws, status = _label(verts, faces, nv, nf)
    cov = torch.empty(V, dtype=torch.int32, device=dev)
    coff = torch.empty(B + 1, dtype=torch.int32, device=dev)
    _lib.call('ofx_mesh_cc_table', _lib.ptr(faces), _lib.ptr(label), _lib.ptr(offs[0]), _lib.ptr(offs[1]), B, V, F,
              _lib.ptr(cov), _lib.ptr(coff), _lib.ptr(ws), _lib.ptr(status), st)
    co = _read_back(coff, status, 'components').tolist()           # the host sync
    K = co[B]
    table = torch.empty(max(K, 1), 8, dtype=torch.int32, device=dev)
    _lib.call('ofx_mesh_cc_stats', _lib.ptr(verts), _lib.ptr(faces), _lib.ptr(label), _lib.ptr(offs[0]),
              _lib.ptr(offs[1]), B, V, F, K, _lib.ptr(table), _lib.ptr(ws), _lib.ptr(status), st)
    box = table[:, :6].contiguous().view(torch.float32)
    cnt = table[:, 6:].to(torch.int64)
    res, vo, fo = [], 0, 0
    for b in range(B):
        cv = cov[vo:vo + nv[b]]
        fb = faces[fo:fo + nf[b]]
        rows = slice(co[b], co[b + 1])
        res.append(dict(comp_of_vert=cv, comp_of_face=cv[fb[:, 0].long()], bbox_min=box[rows, :3],
                        bbox_max=box[rows, 3:], n_verts=cnt[rows, 0], n_faces=cnt[rows, 1]))
        vo += nv[b]
        fo += nf[b]
    return res


def write_obj(path, verts, faces, normals=None):
    """Write one mesh as OBJ -- ``v x y z`` lines, then 1-based ``f a b c`` lines (the layout trimesh's export of the
    reference writes; coordinates with 9 significant digits, which round-trip fp32 exactly).  With ``normals``
    ([V, 3], one per vertex): ``vn x y z`` lines after the vertices and faces as ``f a//a b//b c//c``; without, the
    file is what it always was.  Vectorised: one formatting call per block.  An empty mesh (no faces) writes no file
    and warns; returns whether a file was written."""
    v = verts.detach().cpu().numpy() if torch.is_tensor(verts) else np.asarray(verts)
    f = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
    v = np.ascontiguousarray(v, np.float64).reshape(-1, 3)
    f = np.ascontiguousarray(f, np.int64).reshape(-1, 3) + 1
    if normals is not None:
        n = normals.detach().cpu().numpy() if torch.is_tensor(normals) else np.asarray(normals)
        n = np.ascontiguousarray(n, np.float64).reshape(-1, 3)
        if len(n) != len(v):
            raise ValueError('write_obj: %d normals for %d vertices' % (len(n), len(v)))
    if len(f) == 0:
        warnings.warn('write_obj: empty mesh, %s not written' % path)
        return False
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, 'w') as fh:
        for lo in range(0, len(v), 1 << 16):
            blk = v[lo:lo + (1 << 16)]
            fh.write(('v %.9g %.9g %.9g\n' * len(blk)) % tuple(blk.ravel().tolist()))
        for lo in range(0, len(v) if normals is not None else 0, 1 << 16):
            blk = n[lo:lo + (1 << 16)]
            fh.write(('vn %.9g %.9g %.9g\n' * len(blk)) % tuple(blk.ravel().tolist()))
        for lo in range(0, len(f), 1 << 16):
            blk = f[lo:lo + (1 << 16)]
            if normals is not None:
                fh.write(('f %d//%d %d//%d %d//%d\n' * len(blk)) % tuple(np.repeat(blk.ravel(), 2).tolist()))
            else:
                fh.write(('f %d %d %d\n' * len(blk)) % tuple(blk.ravel().tolist()))
    return True


def read_obj(path):
    """(verts [V, 3] float32, faces [F, 3] int32, 0-based) of an OBJ with ``v`` / triangular ``f`` lines."""
    vs, fs = [], []
    with open(path) as fh:
        for line in fh:
            if line.startswith('v '):
                vs.append(line.split()[1:4])
            elif line.startswith('f '):
                fs.append([t.split('/')[0] for t in line.split()[1:4]])
    v = np.asarray(vs, np.float64).astype(np.float32).reshape(-1, 3)
    f = (np.asarray(fs, np.int64) - 1).astype(np.int32).reshape(-1, 3)
    return v, f


_PLY_XYZ = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
_PLY_NRM = [('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')]


def write_ply(path, points, normals=None):
    """Write a point cloud as binary little-endian PLY: one ``vertex`` element with float32 properties ``x y z`` and,
    with normals, ``nx ny nz`` (the layout of the reference's points2ply, utils/util_dualoctree.py:171-197, and of the
    ``input.ply`` its inference writes).  Vectorised: one array, one write; zero points give a valid header-only
    file."""
    p = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
    cols, props = [p], list(_PLY_XYZ)
    if normals is not None:
        q = normals.detach().cpu().numpy() if torch.is_tensor(normals) else np.asarray(normals)
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 3)
        if len(q) != len(p):
            raise ValueError('write_ply: %d normals for %d points' % (len(q), len(p)))
        cols.append(q)
        props += _PLY_NRM
    head = 'ply\nformat binary_little_endian 1.0\nelement vertex %d\n' % len(p)
    head += ''.join('property float %s\n' % name for name, _ in props) + 'end_header\n'
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, 'wb') as fh:
        fh.write(head.encode('ascii'))
        fh.write(np.concatenate(cols, axis=1).astype('<f4').tobytes())


def read_ply(path):
    """(points [n, 3] float32, normals [n, 3] float32 or None) of a PLY as ``write_ply`` writes it: binary
    little-endian, one vertex element whose properties are all float32 and begin with x y z [nx ny nz]."""
    with open(path, 'rb') as fh:
        raw = fh.read()
    end = raw.find(b'end_header\n')
    if not raw.startswith(b'ply\n') or end < 0:
        raise ValueError('read_ply: %s is not a PLY file' % path)
    lines = raw[:end].decode('ascii').split('\n')
    if 'format binary_little_endian 1.0' not in lines:
        raise ValueError('read_ply: %s is not binary little-endian' % path)
    n, props = None, []
    for ln in lines:
        t = ln.split()
        if t[:2] == ['element', 'vertex']:
            n = int(t[2])
        elif t[:1] == ['element']:
            raise ValueError('read_ply: %s has elements other than vertex' % path)
        elif t[:1] == ['property']:
            if t[1] not in ('float', 'float32'):
                raise ValueError('read_ply: property %s of %s is not float32' % (t[-1], path))
            props.append(t[2])
    if n is None or props[:3] != ['x', 'y', 'z']:
        raise ValueError('read_ply: %s has no x y z vertex properties' % path)
    body = np.frombuffer(raw, '<f4', count=n * len(props), offset=end + len(b'end_header\n')).reshape(n, len(props))
    nrm = body[:, 3:6].copy() if props[3:6] == ['nx', 'ny', 'nz'] else None
    return body[:, :3].copy(), nrm
