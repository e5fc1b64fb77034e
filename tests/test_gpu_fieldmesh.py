"""Field meshing on the GPU (csrc/ofx_fieldmesh.hip, octfusion_amd.mesh.field_mesh) against tests/fieldmesh_oracle.py.

In every case the expected mesh comes from the lattice the EXISTING sweep (ofx_mpu_eval_grid through mpu.calc_sdf)
returns, fed to the CPU oracle -- never from the new code:

  test_ragged_trees      bit-equal vertices / faces / stats in the contract's order on the deep ragged trees of
                         tests/graph_oracle.py (random codes), R in {9, 17, 20, 33, one above 0.9 * 2^de}, margins
                         0 1 2, levels 0 and 0.01; and, order-free, the triangle multiset of the dense
                         mesh.marching_cubes output filtered to active cells
  test_reproducible      two calls bitwise equal; a shape alone equals its slice of the batch call
  test_closed_sphere     an octree built from points on a sphere, codes = the sphere's linearisation: no leaks, equal to
                         the whole dense mesh, closed, Euler characteristic 2, some bricks inactive
  test_beyond_dense      the same sphere at R = 1024: closed, no leaks, peak memory below the dense lattice's 4 R^3
  test_top_of_the_range  the same sphere at R = 2048: 1.6 M active bricks of one shape in one call
  test_groups            a batch cut into groups by active bricks, and again by vertex count, equals the uncut call; a
                         single shape past the count limit is refused
  test_refusals          bad arguments raise with the outputs untouched; a NaN code names the shape
  test_pipeline / _cli   pipeline.sample(field_mesh=True) and generate.py --mesh --field-mesh
  test_reconstruct       reconstruct(field_mesh=True) and reconstruct.py --field-mesh
"""
import ctypes
import json
import math
import os
import types

import numpy as np
import pytest
import torch

import fieldmesh_oracle as F
import graph_oracle as G
import mc_oracle as M
from test_gpu_fullwidth import dev
from test_gpu_graph_tables import Guarded, _dev_tree

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TREES = ('deep_a', 'deep_b_mid', 'deep_c', 'full_face')


# ------------------------------------------------------------------------------------------------ fields
def _octree_of(T):
    """The DevTree's arrays as the Octree-like object mpu.MpuField reads (per-depth views of the device arrays)."""
    oc = T.oc
    return types.SimpleNamespace(
        depth=oc.depth, full_depth=oc.full_depth, batch_size=oc.batch_size,
        children=[T.child[T.ncum[d]:T.ncum[d + 1]] for d in range(oc.depth + 1)],
        keys=[T.key[T.ncum[d]:T.ncum[d + 1]] for d in range(oc.depth + 1)],
        nnum=torch.tensor(T.nnum), nnum_nempty=torch.tensor(T.nne))


_FIELDS = {}


def _field(name):
    """(MpuField with random codes over full_depth .. depth, DevTree) of a named tree."""
    from octfusion_amd import mpu
    if name not in _FIELDS:
        T = _dev_tree(name)
        oc = T.oc
        rows = sum(T.nnum[oc.full_depth:oc.depth + 1])
        rng = np.random.default_rng(sum(map(ord, name)))
        code = rng.standard_normal((rows, 4)).astype(np.float32) * np.array([1, 1, 1, 0.05], np.float32)
        _FIELDS[name] = (mpu.MpuField(oc.full_depth, oc.depth, torch.from_numpy(code).to(dev()), _octree_of(T)), T)
    return _FIELDS[name]


def _nodes(oc, de, b):
    """Depth-de cells [n, 3] of shape b, or None where that depth is dense."""
    if de <= oc.full_depth:
        return None
    x, y, z, bb = G._decode(oc.keys[de].cpu().numpy(), de)
    sel = bb == b
    return np.stack([x[sel], y[sel], z[sel]], 1)


def _dense(field, B, R):
    from octfusion_amd import mpu
    return mpu.calc_sdf(field, B, size=R, bbmin=-0.9, bbmax=0.9)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _check_against_oracle(field, oc, R, sdfs, margins, levels, scale=1.0, dense_too=True):
    from octfusion_amd import mesh
    B, de = oc.batch_size, field.depth_out
    lat = sdfs.cpu().numpy()
    for level in levels:
        dense = mesh.marching_cubes(sdfs, level=level, scale=scale) if dense_too else None
        for m in margins:
            st = {}
            got = mesh.field_mesh(field, R, level=level, scale=scale, margin=m, stats=st)
            assert len(got) == B and st['total_bricks'] == [F.n_bricks(R) ** 3] * B
            for b in range(B):
                v, f, want = F.field_mesh(lat[b], de, _nodes(oc, de, b), margin=m, level=level, scale=scale,
                                               fused=True)
                tag = (R, level, m, b)
                assert (st['seeds'][b], st['bricks'][b], st['leaks'][b]) == \
                    (want['seeds'], want['bricks'], want['leaks']), tag
                gv, gf = got[b]
                assert gv.dtype == torch.float32 and gf.dtype == torch.int32
                assert tuple(gv.shape) == v.shape and tuple(gf.shape) == f.shape, tag
                assert np.array_equal(_bits(gv), v.view(np.uint32)), tag
                assert np.array_equal(gf.cpu().numpy(), f), tag
                if dense_too:                         # order-free, against the dense path's own output
                    dv, df = dense[b][0].cpu().numpy(), dense[b][1].cpu().numpy()
                    cells = F.dense_cells_of_faces(lat[b], level)
                    assert len(cells) == len(df)
                    keep = want['active'][cells[:, 0] // 8, cells[:, 1] // 8, cells[:, 2] // 8]
                    assert np.array_equal(F.canonical_triangles(gv.cpu().numpy(), gf.cpu().numpy()),
                                          F.canonical_triangles(dv, df[keep])), tag


@pytest.mark.parametrize('R', [9, 17, 20, 33, 'big'])
@pytest.mark.parametrize('name', TREES)
def test_ragged_trees(name, R):
    field, T = _field(name)
    oc = T.oc
    if R == 'big':
        R = int(0.9 * 2 ** oc.depth) + 3              # lattice finer than the finest octree cells
    sdfs = _dense(field, oc.batch_size, R)
    _check_against_oracle(field, oc, R, sdfs, (0, 1, 2), (0.0, 0.01))


def test_dense_depth_activates_everything():
    """depth_out <= full_depth: no octree to follow, every brick is active and the mesh is the dense one"""
    from octfusion_amd import mesh, mpu
    field, T = _field('deep_a')
    oc = T.oc
    fd = oc.full_depth
    low = mpu.MpuField(fd, fd, field.reg[:T.nnum[fd]].contiguous(), field.octree)
    sdfs = _dense(low, oc.batch_size, 20)
    _check_against_oracle(low, oc, 20, sdfs, (0,), (0.0,))
    st = {}
    mesh.field_mesh(low, 20, margin=0, stats=st)
    assert st['bricks'] == st['seeds'] == st['total_bricks']


def test_reproducible():
    from octfusion_amd import mesh
    field, T = _field('deep_b_mid')
    B = T.oc.batch_size
    for R, m in ((33, 1), (20, 0)):
        s1, s2 = {}, {}
        a = mesh.field_mesh(field, R, margin=m, scale=0.5, stats=s1)
        b = mesh.field_mesh(field, R, margin=m, scale=0.5, stats=s2)
        assert s1 == s2 and sum(s1['bricks']) > 0
        for (av, af), (bv, bf) in zip(a, b):
            assert torch.equal(av.view(torch.int32), bv.view(torch.int32)) and torch.equal(af, bf)
        for k in range(B):                            # each shape alone, and in another order
            s = {}
            (v, f), = mesh.field_mesh(field, R, margin=m, scale=0.5, shapes=[k], stats=s)
            assert torch.equal(v.view(torch.int32), a[k][0].view(torch.int32)) and torch.equal(f, a[k][1])
            assert (s['seeds'], s['bricks'], s['leaks']) == ([s1['seeds'][k]], [s1['bricks'][k]], [s1['leaks'][k]])
        back = mesh.field_mesh(field, R, margin=m, scale=0.5, shapes=list(range(B))[::-1])
        for k in range(B):
            assert torch.equal(back[B - 1 - k][1], a[k][1])
    # the empty batch element of this tree: an empty mesh, the writer's usual warning
    empty = [k for k in range(B) if a[k][1].shape[0] == 0]
    assert empty and all(a[k][0].shape == (0, 3) for k in empty)
    with pytest.warns(UserWarning, match='empty mesh'):
        assert mesh.write_obj('/nonexistent/never_written.obj', *a[empty[0]]) is False


# ------------------------------------------------------------------------------------------------ the sphere
# Radius 0.47, not 0.5: a sphere of radius 0.5 touches the octree's cell faces x, y, z = +-0.5 of EVERY depth at its
# six poles, the nodes there exist on one side only, and the field grows six thin closed slivers beside the poles that
# a lattice of R <= 256 steps over and a finer one finds (CPU oracle, dense path, R = 320: Euler characteristic 14, area
# +2.0 %).  At 0.47 the dense path's mesh is one sphere at every size tried (oracle: R = 96, 128, 320).
SPHERE_R, SPHERE_DEPTH, SPHERE_FULL = 0.47, 6, 3


def sphere_points(n=200000, r=SPHERE_R):
    """n points on the sphere |x| = r (Fibonacci lattice) and their normals."""
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
    s = np.sqrt(1.0 - z * z)
    nrm = np.stack([s * np.cos(phi), s * np.sin(phi), z], 1).astype(np.float32)
    return nrm * np.float32(r), nrm


def sphere_codes(xyz_per_depth, r=SPHERE_R):
    """The sphere's linearisation at every node centre: c.xyz = x / |x|, c.w = |x| - r.  xyz_per_depth: [(d, x, y, z)]
    integer cell coordinates, depths ascending."""
    rows = []
    for d, x, y, z in xyz_per_depth:
        c = (np.stack([x, y, z], 1).astype(np.float64) + 0.5) * (2.0 / 2 ** d) - 1.0
        n = np.linalg.norm(c, axis=1, keepdims=True)
        rows.append(np.concatenate([c / np.maximum(n, 1e-12), n - r], 1))
    return np.concatenate(rows).astype(np.float32)


_SPHERE = []


def _sphere_field():
    from octfusion_amd import mpu
    from octfusion_amd.octree import Octree, Points
    if not _SPHERE:
        p, n = sphere_points()
        pts = Points(torch.from_numpy(p).to(dev()), torch.from_numpy(n).to(dev()))
        oc = Octree(SPHERE_DEPTH, SPHERE_FULL, 1, dev())
        oc.build_octree(pts)
        per_depth = []
        for d in range(SPHERE_FULL, SPHERE_DEPTH + 1):
            x, y, z, _ = G._decode(oc.keys[d].cpu().numpy(), d)
            per_depth.append((d, x, y, z))
        code = torch.from_numpy(sphere_codes(per_depth)).to(dev())
        _SPHERE.append((mpu.MpuField(SPHERE_FULL, SPHERE_DEPTH, code, oc), oc))
    return _SPHERE[0]


_DENSE_AREA = {}


@pytest.mark.parametrize('R', [96, 128])
def test_closed_sphere(R):
    from octfusion_amd import mesh
    field, oc = _sphere_field()
    sdfs = _dense(field, 1, R)
    lat = sdfs[0].cpu().numpy()
    nodes = _nodes(oc, SPHERE_DEPTH, 0)
    dv, df = M.marching_cubes(lat, 0.0)
    _DENSE_AREA[R] = M.area(dv, df)
    cells = F.dense_cells_of_faces(lat, 0.0)
    gv, gf = (t.cpu().numpy() for t in mesh.marching_cubes(sdfs)[0])         # the dense path's own mesh
    assert np.array_equal(gf, df)
    whole = F.canonical_triangles(gv, gf)
    for m in (0, 1):
        # the precondition, from the dense lattice alone: the dense surface stays inside the band
        act = F.active_bricks(R, SPHERE_DEPTH, nodes, m)
        assert act[cells[:, 0] // 8, cells[:, 1] // 8, cells[:, 2] // 8].all(), 'the dense mesh leaves the band'
        assert not act.all()
        st = {}
        (v, f), = mesh.field_mesh(field, R, margin=m, stats=st)
        assert st['leaks'] == [0] and 0 < st['bricks'][0] < st['total_bricks'][0] and st['bricks'][0] == int(act.sum())
        v, f = v.cpu().numpy(), f.cpu().numpy()
        assert len(v) == len(dv) and len(f) == len(df)
        assert np.array_equal(F.canonical_triangles(v, f), whole)
        assert M.directed_edge_balance(f) and M.euler(v, f) == 2
    # ... and in the contract's order, through the oracle (one margin: the oracle sorts 10^5 triangles)
    _check_against_oracle(field, oc, R, sdfs, (1,), (0.0,), dense_too=False)


def test_beyond_dense():
    """R = 1024, past the dense path's 512: completes, closed, no leaks, never a lattice-sized allocation, and the
    area is the sphere's to within the error the dense path itself shows at R = 128.

    The bound.  The field is a blend of tangent planes of the sphere's distance; a tangent plane under-estimates a
    convex function, so the field's zero set lies slightly OUTSIDE the sphere (area + e_f, the same at every R), while
    marching cubes inscribes triangles in it (area - d(R), d falling with R^-2).  The dense path at R = 128 therefore
    shows |e_f - d(128)|, and a finer lattice shows up to e_f.  The bound is the R = 128 figure plus the most d(128)
    can be: a triangle inside one cell has edges up to the cell diagonal sqrt(3) h, hence (equilateral) a circumradius
    up to h; at its corners its plane is tilted against a sphere of radius r by up to asin(h / r), so it loses at most
    1 - cos = h^2 / (2 r^2) of the area it replaces (h = 1.8 / 128, r = 0.47: 4.5e-4).
    The dense path on the CPU oracle: R = 96 +3.47e-3, R = 128 +3.67e-3, R = 320 +3.96e-3 (e_f ~ 4.0e-3)."""
    from octfusion_amd import mesh
    field, oc = _sphere_field()
    R, scale = 1024, 0.5
    if 128 not in _DENSE_AREA:
        lat = _dense(field, 1, 128)[0].cpu().numpy()
        _DENSE_AREA[128] = M.area(*M.marching_cubes(lat, 0.0))
    true = 4.0 * math.pi * SPHERE_R ** 2
    h = 1.8 / 128
    bound = abs(_DENSE_AREA[128] - true) / true + h * h / (2.0 * SPHERE_R ** 2)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    st = {}
    (v, f), = mesh.field_mesh(field, R, scale=scale, margin=1, stats=st)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(json.dumps({'test': 'fieldmesh_beyond_dense', 'R': R, 'bricks': st['bricks'][0],
                      'total_bricks': st['total_bricks'][0], 'vertices': int(v.shape[0]), 'faces': int(f.shape[0]),
                      'peak_bytes': int(peak), 'dense_lattice_bytes': 4 * R ** 3, 'area_rel_err_bound': bound}))
    assert peak < 4 * R ** 3
    assert st['leaks'] == [0] and st['bricks'][0] < st['total_bricks'][0]
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert M.directed_edge_balance(f) and M.euler(v, f) == 2
    area = M.area(v, f)
    assert abs(area - true * scale ** 2) <= bound * true * scale ** 2, (area, true * scale ** 2, bound)


def test_top_of_the_range():
    """R = 2048, the largest lattice: about 1.6 M of the 16.8 M bricks are active for this one shape, and a shape is
    never cut, so they go through one call.  Completes, closed, no leaks, well below the 34 GB of a dense lattice.
    F - (2 V - 4), printed, is 0 for one closed surface of genus 0."""
    from octfusion_amd import mesh
    field, oc = _sphere_field()
    R = 2048
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    st = {}
    (v, f), = mesh.field_mesh(field, R, margin=1, stats=st)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(json.dumps({'test': 'fieldmesh_top_of_the_range', 'R': R, 'bricks': st['bricks'][0],
                      'total_bricks': st['total_bricks'][0], 'vertices': int(v.shape[0]), 'faces': int(f.shape[0]),
                      'peak_bytes': int(peak), 'dense_lattice_bytes': 4 * R ** 3,
                      'faces_minus_2v_minus_4': int(f.shape[0]) - (2 * int(v.shape[0]) - 4)}))
    assert st['total_bricks'] == [256 ** 3] and 10 ** 6 < st['bricks'][0] < st['total_bricks'][0] // 4
    assert st['leaks'] == [0] and peak < 4 * R ** 3
    f = f.cpu().numpy()
    assert int(f.min()) == 0 and int(f.max()) == v.shape[0] - 1
    assert M.directed_edge_balance(f)
    r = torch.linalg.norm(v, dim=1)                   # every vertex on the sphere, to within the field's own offset
    assert float(r.min()) > SPHERE_R - 1e-3 and float(r.max()) < SPHERE_R + 4e-3


def test_groups(monkeypatch):
    """The host-side cuts of a batch: by active bricks before the count pass, by vertices / triangles after it.  Every
    cut gives the meshes and stats of the uncut call, and a single shape past the count limit is refused."""
    from octfusion_amd import mesh
    field, T = _field('deep_a')
    B = T.oc.batch_size
    s0 = {}
    want = mesh.field_mesh(field, 33, margin=1, stats=s0)
    assert B == 2 and all(n > 1 for n in s0['bricks'])

    def same(got, s):
        assert s == s0
        for (v, f), (wv, wf) in zip(got, want):
            assert torch.equal(v.view(torch.int32), wv.view(torch.int32)) and torch.equal(f, wf)
    calls = []
    real = mesh._field_group
    monkeypatch.setattr(mesh, '_field_group', lambda *a: calls.append((a[3], a[4])) or real(*a))
    s = {}
    monkeypatch.setattr(mesh, 'FIELD_GROUP_BRICKS', max(s0['bricks']))          # each shape alone fits, both do not
    same(mesh.field_mesh(field, 33, margin=1, stats=s), s)
    assert calls == [(0, 1), (1, 1)]
    del calls[:]
    monkeypatch.setattr(mesh, 'FIELD_GROUP_BRICKS', 1)                          # a shape alone may exceed the aim
    same(mesh.field_mesh(field, 33, margin=1, stats=s), s)
    assert calls == [(0, 1), (1, 1)]
    del calls[:]
    monkeypatch.setattr(mesh, 'FIELD_GROUP_BRICKS', 1 << 22)
    nv = [int(v.shape[0]) for v, _ in want]
    nt = [int(f.shape[0]) for _, f in want]
    assert min(nt) > 0 and max(nt) >= max(nv)
    monkeypatch.setattr(mesh, 'FIELD_MAX_COUNT', max(nt))                       # together too many, each alone fits
    same(mesh.field_mesh(field, 33, margin=1, stats=s), s)
    assert calls == [(0, 2), (0, 1), (1, 1)]
    monkeypatch.setattr(mesh, 'FIELD_MAX_COUNT', max(nt) - 1)
    k = nt.index(max(nt))
    with pytest.raises(ValueError, match=r'field_mesh: shape %d has %d vertices and %d triangles' % (k, nv[k], nt[k])):
        mesh.field_mesh(field, 33, margin=1)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from octfusion_amd import _lib, mesh, mpu
    from octfusion_amd._lib import call, stream
    field, T = _field('deep_a')
    oc = T.oc
    B, de, fd = oc.batch_size, oc.depth, oc.full_depth
    for kw in (dict(size=1), dict(size=2049), dict(size=20, level=float('nan')), dict(size=20, level=float('inf')),
               dict(size=20, margin=-1), dict(size=20, shapes=[B]), dict(size=20, bbmin=0.9, bbmax=-0.9)):
        with pytest.raises(ValueError, match='field_mesh'):
            mesh.field_mesh(field, **kw)
    with pytest.raises(ValueError, match='depth_out'):
        mesh.field_mesh(mpu.MpuField(fd, de + 1, field.reg, field.octree), 20)
    with pytest.raises(ValueError, match='MpuField'):
        mesh.field_mesh(lambda p: p, 20)

    # the entry points themselves: every refusal leaves every output untouched
    L = _lib.lib()
    R, step = 20, 1.8 / 20
    assert L.ofx_fieldmesh_classify_ws_bytes(B, 1) == 0 and L.ofx_fieldmesh_classify_ws_bytes(B, 2049) == 0
    assert L.ofx_fieldmesh_classify_ws_bytes(0, R) == 0 and L.ofx_fieldmesh_classify_ws_bytes(129, R) == 0
    assert L.ofx_fieldmesh_ws_bytes(0) == 0 and L.ofx_fieldmesh_ws_bytes(2 ** 26 + 1) == 0
    assert L.ofx_fieldmesh_ws_bytes(1) >= 4404
    tree = ctypes.byref(T.tree)
    cws = Guarded(L.ofx_fieldmesh_classify_ws_bytes(B, R), torch.uint8)
    ws = Guarded(L.ofx_fieldmesh_ws_bytes(64), torch.uint8)
    bc, cnt = Guarded(2 * B, torch.int64), Guarded(4 * B, torch.int64)
    verts, faces = Guarded(3 * 4096, torch.float32), Guarded(3 * 4096, torch.int32)
    offs = torch.zeros(2 * B, dtype=torch.int64, device=dev())
    C = field.reg.data_ptr()
    assert cws.ptr % 16 == 0 and ws.ptr % 16 == 0 and C % 16 == 0

    def refused(name, *args):
        with pytest.raises(_lib.OfxError, match='invalid argument'):
            call(name, *args, stream())

    def classify(de=de, b0=0, nb=B, R=R, step=step, bbmin=-0.9, m=1, cws=cws.ptr, out=bc.ptr, tree=tree):
        refused('ofx_fieldmesh_classify', tree, de, b0, nb, R, step, bbmin, m, cws, out)

    def count(ds=fd, de=de, code=C, b0=0, nb=B, R=R, step=step, level=0.0, cws=cws.ptr, n=64, ws=ws.ptr, out=cnt.ptr,
              tree=tree):
        refused('ofx_fieldmesh_count', tree, ds, de, code, b0, nb, R, step, -0.9, level, cws, n, ws, out)

    def emit(nb=B, R=R, level=0.0, cws=cws.ptr, n=64, ws=ws.ptr, vo=offs.data_ptr(), to=offs[B:].data_ptr(),
             v=verts.ptr, f=faces.ptr):
        refused('ofx_fieldmesh_emit', nb, R, level, step, -0.9, 1.0, cws, n, ws, vo, to, v, f)

    for R_bad in (1, 2049):
        classify(R=R_bad), count(R=R_bad), emit(R=R_bad)
    classify(m=-1)
    classify(de=de + 1), count(de=de + 1), count(ds=de, de=de - 1), count(ds=-1)
    classify(nb=0), classify(nb=B + 1), classify(b0=1), classify(b0=-1), count(nb=B + 1), emit(nb=0), emit(nb=129)
    classify(step=0.0), classify(step=float('nan')), classify(bbmin=float('inf')), count(step=-0.1)
    count(level=float('nan')), emit(level=float('inf'))
    classify(cws=None), classify(out=None), classify(tree=None)
    count(code=None), count(cws=None), count(ws=None), count(out=None), count(tree=None)
    emit(cws=None), emit(ws=None), emit(vo=None), emit(to=None), emit(v=None), emit(f=None)
    classify(cws=cws.ptr + 1), classify(out=bc.ptr + 4)
    count(code=C + 4), count(cws=cws.ptr + 8), count(ws=ws.ptr + 2), count(out=cnt.ptr + 4)
    emit(cws=cws.ptr + 4), emit(ws=ws.ptr + 8), emit(vo=offs.data_ptr() + 4), emit(v=verts.ptr + 2)
    emit(f=faces.ptr + 1)
    count(n=0), count(n=2 ** 26 + 1), emit(n=0), emit(n=2 ** 26 + 1)
    torch.cuda.synchronize()
    for o in (cws, ws, bc, cnt, verts, faces):
        assert o.untouched()

    # a NaN code: the non-finite ValueError names the shape
    bad = field.reg.clone()
    rows_b1 = [int(T.ncum[d]) - int(T.ncum[fd]) for d in range(fd, de + 1)]
    x, y, z, bb = G._decode(oc.keys[de].numpy(), de)
    hit = int(np.nonzero(bb == 1)[0][0])              # a finest node of shape 1
    bad[rows_b1[-1] + hit, 3] = float('nan')
    with pytest.raises(ValueError, match=r'field_mesh: shape 1 has \d+ cells with a non-finite corner'):
        mesh.field_mesh(mpu.MpuField(fd, de, bad, field.octree), 33, margin=2)


# ------------------------------------------------------------------------------------------------ end to end
def _tiny():
    from octfusion_amd import configs, mesh
    configs.CONFIGS['tiny_uncond'] = dict(configs.SNET_UNCOND, model_channels=[32, 32])
    configs.VAES['tiny_uncond'] = configs.VAES['snet_uncond']
    mesh.MESH_SCALES['tiny_uncond'] = mesh.MESH_SCALES['snet_uncond']
    return 'tiny_uncond'


def test_pipeline():
    from octfusion_amd import configs, graph_unet_union as U, mesh, pipeline, synthetic
    from octfusion_amd.graph_vae import GraphVAE
    cfg = dict(configs.SNET_UNCOND, model_channels=[32, 32])
    net = U.UNet3DModel(**{k: v for k, v in dict(cfg, stage_flag='hr').items() if k != 'df_type'})
    net.load_state_dict(synthetic.random_state_dict(net))
    net = net.to(dev()).eval()
    vae = GraphVAE(depth=8, channel_in=4, nout=4, full_depth=4, depth_stop=6, depth_out=8, resblk_type='basic',
                   resblk_num=2, code_channel=16, embed_dim=3)
    vae.load_state_dict(synthetic.random_state_dict(vae))
    vae = vae.to(dev()).eval()
    cs = pipeline.CascadeSampler(net, cfg, vae)
    split = synthetic.shell6_split(2, jitter=True).to(dev())
    out = cs.sample(2, ddim_steps=2, seed=3, split_small=split, sdf_resolution=64, mesh=True, mesh_scale=0.5,
                    field_mesh=True, mesh_margin=1)
    assert 'sdfs' not in out and len(out['meshes']) == 2
    st = {}
    want = mesh.field_mesh(out['decoded']['neural_mpu'], 64, scale=0.5, margin=1, stats=st)
    assert out['mesh_stats'] == st and set(st) == {'seeds', 'bricks', 'leaks', 'total_bricks'}
    for (v, f), (wv, wf) in zip(out['meshes'], want):
        assert f.shape[0] > 0
        assert torch.equal(v.view(torch.int32), wv.view(torch.int32)) and torch.equal(f, wf)
    # the other consumers of a mesh list take it unchanged
    from octfusion_amd import metrics, simplify
    assert metrics.sample_surface(out['meshes'], n=256, seed=0).shape == (2, 256, 3)
    assert len(simplify.simplify(out['meshes'], cells=16)) == 2
    cleaned = cs.sample(2, ddim_steps=2, seed=3, split_small=split, sdf_resolution=64, mesh=True, mesh_scale=0.5,
                        field_mesh=True, mesh_clean=True)
    assert len(cleaned['mesh_components']) == 2 and 'components' not in cleaned['mesh_stats']
    with pytest.raises(ValueError, match='field_mesh needs'):
        cs.sample(2, ddim_steps=2, split_small=split, sdf_resolution=64, field_mesh=True)


def test_cli(tmp_path, capsys):
    from octfusion_amd import generate as Gen, mesh
    out_dir = str(tmp_path / 'gen')
    res = Gen.main(['--config', _tiny(), '--shapes', '2', '--steps', '3', '--batch', '2', '--sdf-resolution', '48',
                    '--seed', '5', '--mesh', '--field-mesh', '--mesh-margin', '2', '--out', out_dir])
    line = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1])
    assert line['mesh_margin'] == 2 and line['rank0_mesh_total_bricks'] == [216, 216]
    for k in ('seeds', 'bricks', 'leaks'):
        assert len(line['rank0_mesh_' + k]) == 2
    for i in range(2):
        assert not os.path.exists(os.path.join(out_dir, str(i), 'sdf.pt'))
        if res['rank0_mesh_faces'][i]:
            v, f = mesh.read_obj(os.path.join(out_dir, '%d.obj' % i))
            assert (len(v), len(f)) == (res['rank0_mesh_vertices'][i], res['rank0_mesh_faces'][i])
    assert sum(res['rank0_mesh_faces']) > 0
    with pytest.raises(ValueError, match='--field-mesh needs --mesh'):
        Gen.main(['--config', _tiny(), '--shapes', '1', '--field-mesh'])


def test_reconstruct(golden, tmp_path):
    """reconstruct(field_mesh=True): the meshes are field_mesh's on the batch's field, the records carry mesh_stats,
    nothing else of the result changes; and the command line's checks."""
    from octfusion_amd import mesh, reconstruct as R, synthetic
    from octfusion_amd.graph_vae import GraphVAE
    kw = dict(golden('g_vae_enc')['cfg'])
    ps = 0.5
    for name, r in (('ball', 0.6), ('pea', 0.35)):
        p, n = sphere_points(4000, r)
        d = tmp_path / 'data' / name
        d.mkdir(parents=True)
        np.savez(str(d / 'pointcloud.npz'), points=p * ps, normals=n)
    vae = GraphVAE(**kw)
    vae.load_state_dict(synthetic.random_state_dict(vae))
    vae = vae.to(dev()).eval()
    cfg = {'depth': kw['depth'], 'full_depth': kw['full_depth'], 'point_scale': ps}
    inputs = R.read_inputs([str(tmp_path / 'data' / 'ball'), str(tmp_path / 'data' / 'pea')])
    out_dir = str(tmp_path / 'recon')
    with pytest.warns(UserWarning):                   # no points.npz beside the inputs; maybe an empty mesh
        res = R.reconstruct(vae, cfg, inputs, dev(), sdf_resolution=40, batch=2, seed=4, chamfer_points=0,
                            out_dir=out_dir, occupancy=True, field_mesh=True, mesh_margin=2)
    assert res['field_mesh'] is True and res['mesh_margin'] == 2 and res['sdf_resolution'] == 40
    saved = json.load(open(os.path.join(out_dir, 'metrics.json')))
    assert saved['field_mesh'] is True and saved['mesh_margin'] == 2
    for name in ('ball', 'pea'):
        field, k = res['fields'][name]
        st = {}
        (wv, wf), = mesh.field_mesh(field, 40, scale=ps, margin=2, shapes=[k], stats=st)
        v, f = res['meshes'][name]
        assert torch.equal(v.view(torch.int32), wv.view(torch.int32)) and torch.equal(f, wf)
        rec = saved['shapes'][name]
        assert rec['mesh_stats'] == {key: val[0] for key, val in st.items()}
        assert rec['mesh_stats']['total_bricks'] == 125
        assert (rec['vertices'], rec['faces']) == (v.shape[0], f.shape[0])
        if rec['faces']:
            rv, rf = mesh.read_obj(os.path.join(out_dir, name, '0.obj'))
            assert np.array_equal(rf, f.cpu().numpy())
    assert sum(saved['shapes'][n]['faces'] for n in ('ball', 'pea')) > 0
    with pytest.warns(UserWarning):
        plain = R.reconstruct(vae, cfg, inputs, dev(), sdf_resolution=40, batch=2, seed=4, chamfer_points=0,
                              occupancy=True)
    assert 'field_mesh' not in plain and all('mesh_stats' not in r for r in plain['shapes'].values())
    base = ['--input', str(tmp_path / 'data' / 'ball'), '--out', out_dir]
    args = R.parse_args(base + ['--field-mesh', '--sdf-resolution', '2048', '--mesh-margin', '0'])
    assert args.field_mesh and args.mesh_margin == 0 and not R.parse_args(base).field_mesh
    for bad in (['--sdf-resolution', '2049'], ['--mesh-margin', '-1']):
        with pytest.raises(ValueError, match='--field-mesh needs'):
            R.parse_args(base + ['--field-mesh'] + bad)
    assert R.parse_args(base + ['--sdf-resolution', '2049']).sdf_resolution == 2049   # the dense path checks later
