"""Mesh export of the generate path: marching cubes on the device (csrc/ofx_mesh.hip) and an OBJ writer.

Replaces the reference's host tail (export_mesh, models/octfusion_model_union.py:435-468; create_mesh,
utils/util_dualoctree.py:120-142): skimage.measure.marching_cubes(sdf, level=0) per shape, vertices mapped by
``vtx * ((bbmax - bbmin) / size) + bbmin`` and ``* point_scale``, written as ``<index>.obj`` by trimesh.

Differences from the reference:
  * the triangulation table is the project's own (tools/gen_mc_table.py): same vertices as skimage (one per crossing
    lattice edge, linear interpolation), but in ambiguous cells the topology may differ from the Lewiner tables;
  * an empty shape is skipped with a warning -- the reference returns at the first empty shape and drops the rest of
    the batch (octfusion_model_union.py:453-455).
"""
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


def mesh_scale(config):
    """The reference's point_scale for a config name of octfusion_amd.configs."""
    return MESH_SCALES[config]


def _max_batch(size):
    return max(1, (2 ** 31 - 1) // (MAX_TRI_PER_CELL * size ** 3))


def marching_cubes(sdfs, level=0.0, bbmin=-0.9, bbmax=0.9, scale=1.0):
    """Meshes of a batch of SDF lattices ``sdfs`` [B, R, R, R] (fp32 on the device, x slowest; what
    ``mpu.calc_sdf`` and the pipeline produce).  Returns a list of B ``(verts [V, 3] fp32, faces [F, 3] int32)``
    device tensors: vertices in ``(index * (bbmax - bbmin) / R + bbmin) * scale`` coordinates, faces 0-based into
    that shape's own vertices, wound so that the normals point to increasing values (outward for an SDF that is
    negative inside).

    Makes ONE host synchronisation: the per-shape counts are read back between the count and the emit pass (once
    per group of ``(2^31 - 1) // (5 R^3)`` shapes -- 25 at R = 256).  Raises ValueError naming the shape if a cell
    of it has a non-finite corner, and OfxError without a GPU (there is no CPU path)."""
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
    g = _max_batch(R)
    for b0 in range(0, B, g):
        out += _group(sdfs[b0:b0 + g], b0, R, float(level), step, float(bbmin), float(scale))
    return out


def _group(sdf, b0, R, level, step, bbmin, scale):
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
    return [(verts[int(voff[b]):int(voff[b] + nv[b])], faces[int(toff[b]):int(toff[b] + nt[b])]) for b in range(B)]


def write_obj(path, verts, faces):
    """Write one mesh as OBJ -- ``v x y z`` lines, then 1-based ``f a b c`` lines (the layout trimesh's export of the
    reference writes; coordinates with 9 significant digits, which round-trip fp32 exactly).  Vectorised: one
    formatting call per block.  An empty mesh (no faces) writes no file and warns; returns whether a file was
    written."""
    v = verts.detach().cpu().numpy() if torch.is_tensor(verts) else np.asarray(verts)
    f = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
    v = np.ascontiguousarray(v, np.float64).reshape(-1, 3)
    f = np.ascontiguousarray(f, np.int64).reshape(-1, 3) + 1
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
        for lo in range(0, len(f), 1 << 16):
            blk = f[lo:lo + (1 << 16)]
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
