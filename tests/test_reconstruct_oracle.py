"""CPU checks of the reconstruction driver's host side: the PLY writer / reader, the float64 Chamfer oracle against
closed forms (tests/recon_oracle.py; the GPU tests compare the device against it), the oracle's face normals, and the
driver's argument parsing, input reading and output naming -- none of which needs a device."""
import os

import numpy as np
import pytest

import recon_oracle as RO


@pytest.mark.parametrize('n', [0, 1, 5, 1000])
@pytest.mark.parametrize('with_normals', [False, True])
def test_ply_round_trip_is_bit_exact(tmp_path, n, with_normals):
    from octfusion_amd import mesh
    rng = np.random.default_rng(n + 17)
    # raw bit patterns that are valid floats, incl. denormals, -0 and huge values: equality is on the bits
    p = rng.standard_normal((n, 3)).astype(np.float32)
    p = p * np.float32(10.0) ** rng.integers(-30, 30, (n, 3)).astype(np.float32)
    if n:
        p[0] = [-0.0, 1e-45, 3.4e38]
    q = rng.standard_normal((n, 3)).astype(np.float32) if with_normals else None
    path = str(tmp_path / 'sub' / 'cloud.ply')
    mesh.write_ply(path, p, q)
    assert open(path, 'rb').read() == RO.ply_bytes(p, q)
    a, b = mesh.read_ply(path)
    assert a.dtype == np.float32 and a.shape == (n, 3) and a.tobytes() == p.tobytes()
    if with_normals:
        assert b.dtype == np.float32 and b.tobytes() == q.tobytes()
    else:
        assert b is None


def test_ply_accepts_tensors_and_rejects_mismatch(tmp_path):
    import torch
    from octfusion_amd import mesh
    p = torch.arange(12, dtype=torch.float32).view(4, 3)
    mesh.write_ply(str(tmp_path / 't.ply'), p, p * 2)
    a, b = mesh.read_ply(str(tmp_path / 't.ply'))
    assert np.array_equal(a, p.numpy()) and np.array_equal(b, 2 * p.numpy())
    with pytest.raises(ValueError):
        mesh.write_ply(str(tmp_path / 'bad.ply'), p, p[:3])
    (tmp_path / 'no.ply').write_bytes(b'solid x\n')
    with pytest.raises(ValueError):
        mesh.read_ply(str(tmp_path / 'no.ply'))


def test_oracle_chamfer_closed_forms():
    """Two unit cubes as surface lattices of spacing h = 1/m.  (1) offset delta < h / 2 along x: every point's nearest
    neighbour is its own copy, both terms are delta^2 x 1e5.  (2) offset exactly 1: the cubes share a face; a point at
    lattice distance i h from that face has its nearest neighbour on it, straight across (the face carries every (y, z)
    of the lattice), so each term is the mean of (i h)^2 over the planes: (m + 1)^2 points on each end plane, 4 m on
    each plane between."""
    m = 8
    h = 1.0 / m
    A = RO.cube_lattice(m)
    assert len(A) == (m + 1) ** 3 - (m - 1) ** 3
    delta = 0.375 * h
    ca, cb = RO.chamfer(A, A + [delta, 0, 0])
    assert ca == pytest.approx(delta ** 2 * 1e5, rel=1e-12) and cb == pytest.approx(delta ** 2 * 1e5, rel=1e-12)
    want = ((m + 1) ** 2 * 1.0 + sum(4 * m * (i * h) ** 2 for i in range(1, m))) / len(A) * 1e5
    ca, cb = RO.chamfer(A, A + [1.0, 0, 0])
    assert ca == pytest.approx(want, rel=1e-12) and cb == pytest.approx(want, rel=1e-12)
    # directed: a subset against the whole -- every point of the subset is in the whole, not the other way round
    sub = A[A[:, 0] == 0.0]
    ca, cb = RO.chamfer(sub, A)                     # a: from A to sub, b: from sub to A
    assert cb == 0.0 and ca > 0.0
    kd = RO.chamfer_kdtree(A, A + [1.0, 0, 0])      # the reference's own arithmetic, where scipy is installed
    if kd is not None:
        assert kd[0] == pytest.approx(want, rel=1e-12) and kd[1] == pytest.approx(want, rel=1e-12)


def test_oracle_normals():
    v, f = RO.cube_mesh(0.5)
    nrm, a2 = RO.face_normals(v, f)
    cen = v[f].mean(1)
    assert np.allclose(a2, 1.0) and np.allclose(np.abs(nrm).max(1), 1.0)
    assert ((nrm * cen).sum(1) > 0).all()                                # outward
    pts, nn, t = RO.sample_surface_oriented(v, f, 500, seed=3, shape=2, normalize=False)
    assert np.array_equal(nn, nrm[t]) and np.allclose(np.abs((pts * nn).sum(1)), 0.5)     # the point lies on its face
    # a zero-area face is never drawn
    f0 = np.concatenate([f[:5], [[1, 1, 2]], f[5:]]).astype(np.int32)
    _, nn0, t0 = RO.sample_surface_oriented(v, f0, 4000, seed=1)
    assert 5 not in set(t0.tolist()) and np.allclose(np.linalg.norm(nn0, axis=1), 1.0)
    for mesh_ in (RO.cube_mesh(), RO.tetrahedron(), RO.height_field()):
        assert RO.min_angles_deg(*mesh_).min() >= 10.0
    assert len(RO.height_field()[1]) == 300


def test_driver_arguments_and_names(tmp_path):
    from octfusion_amd import reconstruct as R
    a = R.parse_args(['--input', 'x/a.obj', 'y/b.obj', '--out', 'o', '--from-mesh'])
    assert a.input == ['x/a.obj', 'y/b.obj'] and a.from_mesh and a.out == 'o'
    assert (a.config, a.vae, a.allow_pickle, a.points, a.fit, a.sdf_resolution, a.clean, a.batch, a.seed, a.mpu_depth,
            a.chamfer_points) == ('snet_uncond', None, False, R.POINTS, None, 256, False, 8, 0, None, R.POINTS)
    a = R.parse_args(['--config', 'obja_uncond', '--vae', 'v.pth', '--allow-pickle', '--input', 'd', '--out', 'o',
                      '--points', '7', '--fit', '0.8', '--sdf-resolution', '64', '--clean', '--batch', '3', '--seed',
                      '9', '--mpu-depth', '6', '--chamfer-points', '11'])
    assert (a.config, a.vae, a.allow_pickle, a.points, a.fit, a.sdf_resolution, a.clean, a.batch, a.seed, a.mpu_depth,
            a.chamfer_points) == ('obja_uncond', 'v.pth', True, 7, 0.8, 64, True, 3, 9, 6, 11)
    with pytest.raises(SystemExit):
        R.parse_args(['--out', 'o'])                                     # --input is required
    with pytest.raises(ValueError):
        R.parse_args(['--input', 'd', '--out', 'o', '--points', '0'])
    assert 'not a value of the reference' in ' '.join(R.parser().format_help().split())
    # names as inference derives them: base name up to the last '.'
    assert R.shape_name('data/02691156/1a04e3') == '1a04e3'
    assert R.shape_name('data/02691156/1a04e3/') == '1a04e3'
    assert R.shape_name('data/02691156/1a04e3/pointcloud.npz') == '1a04e3'
    assert R.shape_name('samples/12.obj') == '12' and R.shape_name('a/b.c.obj') == 'b.c'
    with pytest.raises(ValueError):
        R.shape_name('samples/.obj')                                     # inference's rule would leave ''
    assert R.recon_config('snet_uncond') == {'name': 'snet_uncond', 'depth': 8, 'full_depth': 4, 'point_scale': 0.5}
    assert R.recon_config('obja_uncond')['point_scale'] == 1.0
    # reading: both kinds, no device
    from octfusion_amd import mesh
    v, f = RO.cube_mesh(0.3)
    mesh.write_obj(str(tmp_path / 'box.obj'), v, f)
    d = tmp_path / 'shape0'
    d.mkdir()
    pts = np.arange(12, dtype=np.float64).reshape(4, 3) / 40
    np.savez(str(d / 'pointcloud.npz'), points=pts, normals=np.ones((4, 3)))
    got = R.read_inputs([str(d), str(tmp_path / 'box.obj')][:1])
    assert got[0]['name'] == 'shape0' and got[0]['kind'] == 'points' and got[0]['points'].dtype == np.float32
    assert np.array_equal(got[0]['points'], pts.astype(np.float32))
    got = R.read_inputs([str(tmp_path / 'box.obj')], from_mesh=True)
    assert got[0]['name'] == 'box' and got[0]['kind'] == 'mesh' and np.array_equal(got[0]['faces'], f)
    with pytest.raises(ValueError):
        R.read_inputs([str(d), str(d) + os.sep])                         # the same name twice
    with pytest.raises(ValueError):
        R.read_inputs([str(d)], from_mesh=True)                          # --from-mesh wants .obj files


def test_reconstruct_does_not_import_the_oracle():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, 'octfusion_amd', 'reconstruct.py')).read()
    assert not re.search(r'^\s*(from|import)\s+oracle\b', txt, flags=re.M)
