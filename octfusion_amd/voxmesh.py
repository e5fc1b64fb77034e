"""Voxel meshes of generated octrees on the device (csrc/ofx_voxmesh.hip).

Replaces the reference's octree export (export_octree, models/octfusion_model_union.py:403-422; voxel2mesh /
_voxel2mesh, models/networks/diffusion_networks/ldm_diffusion_util.py:345-446): every node of one depth is marked in a
dense float grid, a Python loop over the occupied voxels emits one quad (two triangles) for each cube face whose
neighbour is empty, and trimesh writes ``<save_dir>/octree/<index>.obj``.  Here occupancy is one bit per cell and the
mesh comes from popcounts and a scan; no dense grid is built for an octree.
"""
import torch

from . import _lib

MAX_DEPTH = 8           # include/ofx.h: batch * R^3 * 24 <= INT32_MAX leaves no room for depth 9
_BOUND = 24             # 6 quads = 12 triangles = 24 unwelded vertices per cell through one int32 scan
MAX_BATCH = 65535       # shapes per call of the library (include/ofx.h: a grid dimension of the dense fill)


def _max_batch(R):
    return min(MAX_BATCH, max(1, (2 ** 31 - 1) // (_BOUND * R ** 3)))


def _depth_of(R, who):
    d = int(R).bit_length() - 1
    if R < 2 or (1 << d) != R:
        raise ValueError('%s: grid size %d is not a power of two >= 2' % (who, R))
    if d > MAX_DEPTH:
        raise ValueError('%s: grid size %d above %d' % (who, R, 1 << MAX_DEPTH))
    return d


def voxel_mesh(occ, threshold=0.4, weld=True):
    """Cube-face meshes of occupancy grids ``occ`` [B, R, R, R] or [R, R, R] (fp32 on the device, x slowest, R a power
    of two up to 256): a cell is occupied where its value is > ``threshold``, and every face of an occupied cell whose
    neighbour is empty or outside the grid becomes one quad of two outward-wound triangles.  Returns what
    ``mesh.marching_cubes`` returns -- a list of B ``(verts [V, 3] fp32, faces [F, 3] int32)`` device tensors, faces
    0-based into that shape's own vertices -- so ``mesh.write_obj``, ``mesh.largest_component``, ``mesh.components``
    and ``metrics.sample_surface`` take it as it is.  Vertices are ``corner * 2 / R - 1`` (the cube [-1, 1]^3, exact in
    fp32); quads in the reference's order: cells ascending in (x, y, z), within a cell +z, -z, -x, +x, +y, -y.  An
    empty grid gives empty tensors.  Bitwise reproducible.

    ONE host synchronisation per group of ``min(65535, (2^31 - 1) // (24 R^3))`` shapes (the per-shape counts, read
    back between the count and the emit pass).  Raises ValueError for a wrong dtype, device or shape or a non-power-of-two R, and
    OfxError without a GPU (there is no CPU path).

    Choices:
      * weld=True is the default: every lattice corner a quad uses appears once, in ascending corner index
        ``(cx (R + 1) + cy) (R + 1) + cz``.  Without welding every quad has four vertices of its own, so nothing is
        connected and ``components`` / ``clean`` are meaningless; trimesh too merges coincident vertices when the
        reference constructs its mesh.  weld=False gives the arrays of the reference's ``_voxel2mesh`` verbatim, order
        included (verts in fp32; the float64 values are exact in it).
      * a neighbour whose value EQUALS the threshold counts as empty here and gets a face; the reference emits none
        toward it (it tests ``< threshold``), leaving a hole.
      * non-finite values count as empty (in the reference +inf is occupied and a NaN neighbour gets no face)."""
    _lib.require_device()
    if not torch.is_tensor(occ) or occ.dim() not in (3, 4):
        raise ValueError('voxel_mesh: occ must be a [B, R, R, R] or [R, R, R] tensor')
    if occ.dim() == 3:
        occ = occ[None]
    if not (occ.shape[1] == occ.shape[2] == occ.shape[3]) or occ.shape[0] < 1:
        raise ValueError('voxel_mesh: occ must be [B, R, R, R], got %s' % (tuple(occ.shape),))
    if occ.device.type != 'cuda' or occ.dtype != torch.float32:
        raise ValueError('voxel_mesh: occ must be a float32 device tensor')
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError('voxel_mesh: threshold is NaN')
    B, R = int(occ.shape[0]), int(occ.shape[1])
    depth = _depth_of(R, 'voxel_mesh')
    occ = occ.contiguous()
    out = []
    g = _max_batch(R)
    for b0 in range(0, B, g):
        part = occ[b0:b0 + g]

        def fill(ws, n, part=part):
            _lib.call('ofx_voxmesh_mask_dense', _lib.ptr(part), n, depth, threshold, _lib.ptr(ws), _lib.stream())
        out += _group(fill, int(part.shape[0]), depth, bool(weld), occ.device)
    return out


def octree_mesh(octree, depth, weld=True):
    """``voxel_mesh`` of the nodes of ``octree`` (octfusion_amd.octree.Octree) at ``depth``, empty and non-empty alike
    (the reference's export_octree: ``nempty=False``), on the 2^depth grid: one mesh per shape of the octree's batch.
    The keys are decoded on the device straight into the bitmask; no dense grid is built.  Same result as
    ``voxel_mesh`` of a grid with ones at ``octree.xyzb(depth)``, same return type, ``weld`` and errors; ValueError
    also for a depth the octree does not have."""
    _lib.require_device()
    depth = int(depth)
    if not 1 <= depth <= min(octree.depth, len(octree.keys) - 1) or octree.keys[depth] is None:
        raise ValueError('octree_mesh: the octree has no depth %d' % depth)
    if depth > MAX_DEPTH:
        raise ValueError('octree_mesh: depth %d above %d' % (depth, MAX_DEPTH))
    keys = octree.key(depth)
    if keys.device.type != 'cuda' or keys.dtype != torch.int64:
        raise ValueError('octree_mesh: the keys must be an int64 device tensor')
    keys = keys.contiguous()
    B = int(octree.batch_size)
    out = []
    g = _max_batch(1 << depth)
    for b0 in range(0, B, g):
        def fill(ws, n, b0=b0):
            _lib.call('ofx_voxmesh_mask_keys', _lib.ptr(keys), int(keys.shape[0]), b0, n, depth, _lib.ptr(ws),
                      _lib.stream())
        out += _group(fill, min(g, B - b0), depth, bool(weld), keys.device)
    return out


def _group(fill, B, depth, weld, dev):
    st = _lib.stream()
    nbytes = _lib.lib().ofx_voxmesh_ws_bytes(B, depth, int(weld))
    if nbytes == 0:
        raise ValueError('voxel mesh: %d shapes at depth %d outside the int32 bound' % (B, depth))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    fill(ws, B)
    counts = torch.empty(B * 2, dtype=torch.int64, device=dev)
    _lib.call('ofx_voxmesh_count', B, depth, int(weld), _lib.ptr(ws), _lib.ptr(counts), st)
    c = counts.view(B, 2).cpu()                        # the host sync
    nq = c[:, 0]
    nv = c[:, 1] if weld else 4 * nq
    nt = 2 * nq
    voff = torch.cumsum(nv, 0) - nv
    toff = torch.cumsum(nt, 0) - nt
    V, T = int(nv.sum()), int(nt.sum())
    verts = torch.empty(max(V, 1), 3, dtype=torch.float32, device=dev)
    faces = torch.empty(max(T, 1), 3, dtype=torch.int32, device=dev)
    if T:
        offs = torch.stack([voff, toff]).to(dev)
        _lib.call('ofx_voxmesh_emit', B, depth, int(weld), _lib.ptr(ws), _lib.ptr(offs[0]), _lib.ptr(offs[1]),
                  _lib.ptr(verts), _lib.ptr(faces), st)
    return [(verts[int(voff[b]):int(voff[b] + nv[b])], faces[int(toff[b]):int(toff[b] + nt[b])]) for b in range(B)]
