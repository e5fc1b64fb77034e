"""Marching cubes on the CPU: the numpy oracle (tests/mc_oracle.py) pinned by table-independent geometric facts, the
library's table read through ofx_mc_table_host, the OBJ writer, the no-GPU failure and the config scales."""
import ctypes
import time

import numpy as np
import pytest
import torch

import mc_oracle as M


def test_vertex_count_is_the_number_of_sign_changing_edges():
    for R, f in ((17, M.sphere(17)), (24, M.torus(24)), (20, M.gaussians(20, seed=3)), (9, M.random_signs(9, 1, False))):
        inside = f < 0
        n = int((inside[1:] != inside[:-1]).sum() + (inside[:, 1:] != inside[:, :-1]).sum() +
                (inside[:, :, 1:] != inside[:, :, :-1]).sum())
        v, _ = M.marching_cubes(f)
        assert len(v) == n, R


def test_vertices_lie_on_their_edges_in_lattice_order():
    f = M.gaussians(16, seed=1)
    R = 16
    step = np.float32(1.8 / R)
    v, _ = M.marching_cubes(f, bbmin=-0.9, bbmax=0.9, scale=1.0)
    idx = (v + 0.9) / step                                      # back to index space
    frac = idx - np.floor(idx + 1e-4)
    off_axis = (frac > 1e-3).sum(1)
    assert (off_axis <= 1).all()                                # on a lattice edge
    owner = np.floor(idx + 1e-4).astype(np.int64)
    lin = (owner[:, 0] * R + owner[:, 1]) * R + owner[:, 2]
    assert (np.diff(lin) >= 0).all()                            # ordered by owner


def test_closed_on_random_sign_fields_all_256_cases():
    cases = set()
    for s in range(300):
        R = 6 + s % 4
        f = M.random_signs(R, seed=s)
        cases |= set(M.cube_index(f < 0).ravel().tolist())
        v, faces = M.marching_cubes(f)
        assert M.directed_edge_balance(faces), s
        assert faces.dtype == np.int32 and (faces >= 0).all() and (faces < len(v)).all()
    assert len(cases) == 256


def test_sphere_geometry():
    R, r = 64, 0.5
    f = M.sphere(R, r)
    v, faces = M.marching_cubes(f)
    step = 1.8 / R
    d = np.linalg.norm(v.astype(np.float64) - np.array([0.013, -0.021, 0.007]), axis=1)
    assert np.abs(d - r).max() < step
    vol = M.signed_volume(v, faces)
    assert vol > 0 and abs(vol / (4 / 3 * np.pi * r ** 3) - 1) < 0.01
    assert abs(M.area(v, faces) / (4 * np.pi * r * r) - 1) < 0.02
    assert M.euler(v, faces) == 2
    assert M.directed_edge_balance(faces)


def test_torus_and_scale():
    f = M.torus(64)
    v, faces = M.marching_cubes(f)
    assert M.euler(v, faces) == 0 and M.directed_edge_balance(faces) and M.signed_volume(v, faces) > 0
    v2, faces2 = M.marching_cubes(f, scale=0.5)
    assert np.array_equal(faces, faces2) and np.allclose(v2, v * 0.5, atol=1e-7)


def test_winding_points_to_increasing_values():
    # an SDF that is POSITIVE inside flips every triangle: negative signed volume
    v, faces = M.marching_cubes(-M.sphere(32))
    assert M.signed_volume(v, faces) < 0


def test_boundary_is_not_padded():
    f = M.sphere(24, r=0.95)                                   # reaches the lattice faces
    _, faces = M.marching_cubes(f)
    assert len(faces) and not M.directed_edge_balance(faces)


def test_library_table_equals_the_oracle():
    from octfusion_amd import build, _lib
    build.build()
    tri = (ctypes.c_int8 * (256 * 16))()
    ntri = (ctypes.c_uint8 * 256)()
    assert _lib.call('ofx_mc_table_host', ctypes.addressof(tri), ctypes.addressof(ntri)) == 0
    want_tri, want_n = M.tables()
    assert np.array_equal(np.frombuffer(tri, np.int8).reshape(256, 16), want_tri)
    assert np.array_equal(np.frombuffer(ntri, np.uint8), want_n)
    assert _lib.lib().ofx_mc_ws_bytes(8, 256) > 256 ** 3 * 4
    assert _lib.lib().ofx_mc_ws_bytes(1, 1) == 0 and _lib.lib().ofx_mc_ws_bytes(1, 513) == 0


def test_generated_header_is_up_to_date():
    import gen_mc_table
    import os
    assert open(gen_mc_table.OUT).read() == gen_mc_table.render()
    assert os.path.basename(gen_mc_table.OUT) == 'ofx_mc_table.h'


def test_write_obj_round_trip(tmp_path):
    from octfusion_amd import mesh
    v, faces = M.marching_cubes(M.torus(40), scale=0.5)
    p = str(tmp_path / 'a' / '3.obj')
    assert mesh.write_obj(p, torch.from_numpy(v), torch.from_numpy(faces))
    v2, f2 = mesh.read_obj(p)
    assert np.array_equal(v2, v) and np.array_equal(f2, faces)
    lines = open(p).read().splitlines()
    assert lines[0].startswith('v ') and lines[-1].startswith('f ') and len(lines) == len(v) + len(faces)
    assert min(int(t) for l in lines if l.startswith('f ') for t in l.split()[1:]) == 1      # 1-based


def test_write_obj_empty_mesh_warns_and_writes_nothing(tmp_path):
    from octfusion_amd import mesh
    p = tmp_path / '0.obj'
    with pytest.warns(UserWarning, match='empty mesh'):
        assert mesh.write_obj(str(p), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)) is False
    assert not p.exists()


def test_write_obj_is_vectorised(tmp_path):
    from octfusion_amd import mesh
    rng = np.random.default_rng(0)
    v = rng.random((500_000, 3), dtype=np.float32)
    f = rng.integers(0, len(v), (1_000_000, 3)).astype(np.int32)
    t = time.perf_counter()
    mesh.write_obj(str(tmp_path / 'big.obj'), v, f)
    assert time.perf_counter() - t < 1.5


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_marching_cubes_fails_loudly_without_gpu():
    from octfusion_amd import _lib, mesh
    with pytest.raises(_lib.OfxError):
        mesh.marching_cubes(torch.zeros(1, 8, 8, 8))


def test_config_mesh_scales():
    from octfusion_amd import configs, mesh
    assert mesh.mesh_scale('snet_uncond') == 0.5 and mesh.mesh_scale('snet_cond') == 0.5
    assert mesh.mesh_scale('obja_uncond') == 1.0
    assert set(mesh.MESH_SCALES) == set(configs.CONFIGS)
