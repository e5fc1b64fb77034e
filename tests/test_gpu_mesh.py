"""Marching cubes on the device (csrc/ofx_mesh.hip through octfusion_amd.mesh) against the numpy oracle
(tests/mc_oracle.py): faces equal, vertices within 1e-6 of the bbox extent; determinism, closedness, the non-finite
error, and the generate driver's --mesh end to end."""
import json
import os

import numpy as np
import pytest
import torch

import mc_oracle as M

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

EXTENT = 1.8          # bbmax - bbmin of the default frame [-0.9, 0.9]


def dev():
    return torch.device('cuda:0')


def check(mesh_gpu, field, level=0.0, scale=1.0, bbmin=-0.9, bbmax=0.9):
    v, f = mesh_gpu
    wv, wf = M.marching_cubes(field, level=level, bbmin=bbmin, bbmax=bbmax, scale=scale)
    assert v.dtype == torch.float32 and f.dtype == torch.int32
    assert tuple(v.shape) == wv.shape and tuple(f.shape) == wf.shape
    assert torch.equal(f.cpu(), torch.from_numpy(wf))
    if len(wv):
        assert float((v.cpu() - torch.from_numpy(wv)).abs().max()) <= 1e-6 * (bbmax - bbmin) * abs(scale)
    return wv, wf


def run(fields, **kw):
    from octfusion_amd import mesh
    x = torch.from_numpy(np.stack(fields)).to(dev())
    return mesh.marching_cubes(x, **kw)


@pytest.mark.parametrize('R', [2, 3, 17, 64, 129])
def test_fields_match_the_oracle(R):
    fields = [M.sphere(R, r=0.5), M.torus(R), M.gaussians(R, seed=R)]
    if R == 2:
        fields.append(np.array([[[-1, 1], [1, 1]], [[1, 1], [1, -0.5]]], np.float32))
    out = run(fields)
    assert len(out) == len(fields)
    for m, f in zip(out, fields):
        check(m, f)


def test_random_signs_33():
    fields = [M.random_signs(33, seed=s, border=s == 0) for s in range(3)]
    for m, f in zip(run(fields), fields):
        check(m, f)


def test_size_256_batch_2():
    fields = [M.sphere(256, r=0.6), M.gaussians(256, seed=4)]
    out = run(fields, scale=0.5)
    for m, f in zip(out, fields):
        wv, wf = check(m, f, scale=0.5)
        assert len(wf) > 100_000


def test_empty_and_full_shapes_in_a_batch():
    R = 40
    fields = [np.ones((R, R, R), np.float32), M.torus(R), -np.ones((R, R, R), np.float32)]
    out = run(fields)
    assert [int(v.shape[0]) for v, _ in out][0::2] == [0, 0] and [int(f.shape[0]) for _, f in out][0::2] == [0, 0]
    check(out[1], fields[1])


def test_level_and_frame():
    f = M.gaussians(48, seed=9)
    for m, lev in zip(run([f, f], level=0.1, bbmin=-1.0, bbmax=1.0, scale=2.0), (0.1, 0.1)):
        check(m, f, level=lev, bbmin=-1.0, bbmax=1.0, scale=2.0)
    (v0, f0), = run([f])
    (v1, f1), = run([f], level=-0.05)
    assert f0.shape != f1.shape


def test_bitwise_reproducible_and_closed():
    fields = [M.gaussians(96, seed=2), M.random_signs(96, seed=7), M.torus(96)]
    a, b = run(fields), run(fields)
    for (va, fa), (vb, fb), fld in zip(a, b, fields):
        assert torch.equal(va, vb) and torch.equal(fa, fb)
        assert M.directed_edge_balance(fa.cpu().numpy())
    (v, f), = run([M.sphere(64)])
    assert M.euler(v.cpu().numpy(), f.cpu().numpy()) == 2 and M.signed_volume(v.cpu().numpy(), f.cpu().numpy()) > 0


def test_non_finite_raises_naming_the_shape():
    R = 20
    fields = [M.sphere(R), M.sphere(R), M.torus(R)]
    fields[1][5, 6, 7] = np.nan
    with pytest.raises(ValueError, match='shape 1'):
        run(fields)
    fields[1][5, 6, 7] = np.inf
    with pytest.raises(ValueError, match='shape 1 has 8 cells'):
        run(fields)


def test_generate_cli_writes_obj(tmp_path, capsys):
    from octfusion_amd import configs, generate as G, mesh
    configs.CONFIGS['tiny_uncond'] = dict(configs.SNET_UNCOND, model_channels=[32, 32])
    configs.VAES['tiny_uncond'] = configs.VAES['snet_uncond']
    mesh.MESH_SCALES['tiny_uncond'] = mesh.MESH_SCALES['snet_uncond']
    out_dir = str(tmp_path / 'gen')
    res = G.main(['--config', 'tiny_uncond', '--shapes', '3', '--steps', '4', '--batch', '2', '--sdf-resolution', '64',
                  '--seed', '5', '--mesh', '--out', out_dir])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1]
    assert json.loads(line)['rank0_mesh_faces'] == res['rank0_mesh_faces']
    assert res['rank0_phase_seconds']['mesh'] > 0 and len(res['rank0_mesh_vertices']) == 3
    written = 0
    for k, i in enumerate(res['rank0_indices']):
        sdf = torch.load(os.path.join(out_dir, str(i), 'sdf.pt')).numpy()
        wv, wf = M.marching_cubes(sdf, bbmin=-0.9, bbmax=0.9, scale=0.5)
        assert (res['rank0_mesh_vertices'][k], res['rank0_mesh_faces'][k]) == (len(wv), len(wf))
        p = os.path.join(out_dir, '%d.obj' % i)
        if len(wf) == 0:
            assert not os.path.exists(p)
            continue
        v, f = mesh.read_obj(p)
        assert np.array_equal(f, wf) and np.abs(v - wv).max() <= 1e-6 * 1.8 * 0.5
        written += 1
    assert written > 0
