"""Mesh components and the largest-component clean on the device (csrc/ofx_mesh_cc.hip through octfusion_amd.mesh)
against the numpy / scipy oracle (tests/cc_oracle.py).  Everything is compared exactly."""
import json
import os

import numpy as np
import pytest
import torch

import cc_oracle as C
import mc_oracle as M

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def dev():
    return torch.device('cuda:0')


def mc(fields, **kw):
    from octfusion_amd import mesh
    return mesh.marching_cubes(torch.from_numpy(np.stack(fields)).to(dev()), **kw)


def to_dev(v, f):
    return torch.from_numpy(np.ascontiguousarray(v)).to(dev()), torch.from_numpy(np.ascontiguousarray(f)).to(dev())


def host(m):
    return m[0].cpu().numpy(), m[1].cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def status_clear():
    from octfusion_amd import mesh
    assert mesh.last_cc_status() == (0, 0)


def check_components(meshes):
    from octfusion_amd import mesh
    got = mesh.components(meshes)
    status_clear()
    assert len(got) == len(meshes)
    tabs = []
    for g, m in zip(got, meshes):
        v, f = host(m)
        t = C.table(v, f)
        assert g['comp_of_vert'].dtype == torch.int32 and g['comp_of_face'].dtype == torch.int32
        assert g['n_verts'].dtype == torch.int64 and g['bbox_min'].dtype == torch.float32
        assert np.array_equal(g['comp_of_vert'].cpu().numpy(), t['comp_of_vert'])
        assert np.array_equal(g['comp_of_face'].cpu().numpy(), t['comp_of_face'])
        assert tuple(g['bbox_min'].shape) == t['bbox_min'].shape
        assert np.array_equal(bits(g['bbox_min'].cpu().numpy()), bits(t['bbox_min']))
        assert np.array_equal(bits(g['bbox_max'].cpu().numpy()), bits(t['bbox_max']))
        assert np.array_equal(g['n_verts'].cpu().numpy(), t['n_verts'])
        assert np.array_equal(g['n_faces'].cpu().numpy(), t['n_faces'])
        tabs.append(t)
    return tabs


def check_clean(meshes, cleaned, tabs=None):
    assert len(cleaned) == len(meshes)
    for k, (m, c) in enumerate(zip(meshes, cleaned)):
        v, f = host(m)
        t = tabs[k] if tabs else C.table(v, f)
        cv, cf = host(c)
        assert c[0].dtype == torch.float32 and c[1].dtype == torch.int32
        w = C.select(t)
        if w < 0:
            assert len(cv) == 0 and len(cf) == 0
            continue
        wv, wf = C.extract(v, f, w, t)
        assert np.array_equal(cf, wf)
        assert np.array_equal(bits(cv), bits(wv))              # the kept rows of the uncleaned device mesh


def full_check(fields):
    from octfusion_amd import mesh
    meshes = mc(fields)
    tabs = check_components(meshes)
    a = mesh.largest_component(meshes)
    status_clear()
    check_clean(meshes, a, tabs)
    stats = {}
    b = mc(fields, clean=True, stats=stats)
    status_clear()
    assert stats['components'] == [len(t['n_verts']) for t in tabs]
    for (va, fa), (vb, fb) in zip(a, b):
        assert torch.equal(va, vb) and torch.equal(fa, fb)
    return meshes, tabs, a


@pytest.mark.parametrize('R', [17, 64, 129])
def test_fields_match_the_oracle(R):
    full_check([M.sphere(R, r=0.5), M.torus(R), M.gaussians(R, seed=R)])


def test_two_spheres_and_rod_and_ball():
    _, tabs, a = full_check([C.two_spheres(64)])
    assert len(tabs[0]['n_verts']) == 2
    v, f = host(a[0])
    assert M.directed_edge_balance(f) and M.euler(v, f) == 2
    _, tabs, a = full_check([C.rod_and_ball(96)])
    assert int(a[0][1].shape[0]) == 2768                      # the long thin rod, not the ball with 21 652 faces


def test_random_signs_33():
    full_check([M.random_signs(33, seed=s, border=s == 0) for s in range(3)])


def test_random_signs_96():
    _, tabs, _ = full_check([M.random_signs(96, seed=7)])
    assert len(tabs[0]['n_verts']) == 8089


def test_noisy_128_and_reproducible():
    from octfusion_amd import mesh
    meshes, tabs, a = full_check([C.noisy(128, 3)])
    assert len(tabs[0]['n_verts']) == 136800
    b = mesh.largest_component(meshes)
    assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[0][1], b[0][1])
    t1, t2 = mesh.components(meshes)[0], mesh.components(meshes)[0]
    for key in t1:
        assert torch.equal(t1[key], t2[key]), key
    status_clear()


def test_mixed_batch():
    R = 64
    fields = [np.ones((R, R, R), np.float32), -np.ones((R, R, R), np.float32), M.sphere(R), C.noisy(R, 5)]
    meshes, tabs, a = full_check(fields)
    assert [int(f.shape[0]) for _, f in a][:2] == [0, 0] and [int(v.shape[0]) for v, _ in a][:2] == [0, 0]
    assert len(tabs[0]['n_verts']) == 0 and len(tabs[2]['n_verts']) == 1 and len(tabs[3]['n_verts']) > 10
    assert torch.equal(a[2][0], meshes[2][0]) and torch.equal(a[2][1], meshes[2][1])
    assert 0 < a[3][1].shape[0] < meshes[3][1].shape[0]


def test_deep_chains_on_a_permuted_strip():
    from octfusion_amd import mesh
    n = 200_000
    v, f = C.strip(n, seed=11)
    m = [to_dev(v, f)]
    t = check_components(m)[0]
    assert t['n_faces'].tolist() == [n] and t['n_verts'].tolist() == [n + 2]
    out = mesh.largest_component(m)
    status_clear()
    assert torch.equal(out[0][0], m[0][0]) and torch.equal(out[0][1], m[0][1])
    v, f = C.strip(n, seed=11, cut=n // 2)
    m = [to_dev(v, f)]
    t = check_components(m)[0]
    assert sorted(t['n_faces'].tolist()) == [n // 2 - 2, n // 2]
    assert sorted(t['n_verts'].tolist()) == [n // 2, n // 2 + 2]
    check_clean(m, mesh.largest_component(m), [t])
    status_clear()


def test_tie_rule_unused_vertices_and_batches_of_foreign_meshes():
    from octfusion_amd import mesh
    v, f = C.tetra_pair()
    v2 = np.concatenate([np.full((1, 3), 9, np.float32), v[4:], v[:4]])     # vertex 0 unused, copies swapped
    m = [to_dev(v, f), to_dev(v2, f + 1), to_dev(np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int32))]
    tabs = check_components(m)
    assert tabs[1]['comp_of_vert'][0] == -1
    out = mesh.largest_component(m)
    check_clean(m, out, tabs)
    assert np.array_equal(host(out[0])[0], v[:4]) and np.array_equal(host(out[1])[0], v2[1:5])
    assert out[2][0].shape[0] == 0 and out[2][1].shape[0] == 0
    empty = mesh.components([m[2]])[0]
    assert empty['n_verts'].shape[0] == 0 and empty['comp_of_vert'].tolist() == [-1, -1, -1]


def test_input_checks():
    from octfusion_amd import mesh
    v, f = C.tetra_pair()
    dv, df = to_dev(v, f)
    hi = f.copy()
    hi[5, 1] = 8                                                           # == V
    lo = f.copy()
    lo[0, 0] = -1
    for b in (hi, lo):
        for fn in (mesh.largest_component, mesh.components):
            with pytest.raises(ValueError, match='face index'):
                fn([(dv, df), (dv, torch.from_numpy(b).to(dev()))])
            assert mesh.last_cc_status() == (0, 1)
    for fn in (mesh.largest_component, mesh.components):
        with pytest.raises(ValueError):
            fn([(dv, df.long())])
        with pytest.raises(ValueError):
            fn([(dv.double(), df)])
        with pytest.raises(ValueError):
            fn([(dv.cpu(), df.cpu())])
    mesh.largest_component([(dv, df)])
    status_clear()


def _tiny():
    from octfusion_amd import configs, mesh
    configs.CONFIGS['tiny_uncond'] = dict(configs.SNET_UNCOND, model_channels=[32, 32])
    configs.VAES['tiny_uncond'] = configs.VAES['snet_uncond']
    mesh.MESH_SCALES['tiny_uncond'] = mesh.MESH_SCALES['snet_uncond']


def test_generate_cli_clean(tmp_path, capsys):
    from octfusion_amd import generate as G, mesh
    _tiny()
    out_dir = str(tmp_path / 'gen')
    res = G.main(['--config', 'tiny_uncond', '--shapes', '3', '--steps', '4', '--batch', '2', '--sdf-resolution', '64',
                  '--seed', '5', '--mesh', '--clean', '--points', '256', '--out', out_dir])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1]
    assert json.loads(line)['rank0_mesh_components'] == res['rank0_mesh_components']
    written = 0
    for k, i in enumerate(res['rank0_indices']):
        sdf = torch.load(os.path.join(out_dir, str(i), 'sdf.pt')).numpy()
        wv, wf, comps = C.clean(*M.marching_cubes(sdf, bbmin=-0.9, bbmax=0.9, scale=0.5))
        assert res['rank0_mesh_components'][k] == comps
        assert (res['rank0_mesh_vertices'][k], res['rank0_mesh_faces'][k]) == (len(wv), len(wf))
        p = os.path.join(out_dir, '%d.obj' % i)
        if len(wf) == 0:
            assert not os.path.exists(p)
            continue
        v, f = mesh.read_obj(p)
        assert np.array_equal(f, wf) and np.abs(v - wv).max() <= 1e-6 * 1.8 * 0.5
        assert len(C.table(v, f)['n_verts']) == 1
        # the cloud was sampled from the cleaned mesh: inside its box after the unit-cube normalisation
        pts = np.load(os.path.join(out_dir, '%d.npy' % i))
        assert pts.shape == (256, 3)
        centre, ext = (v.max(0) + v.min(0)) / 2, float((v.max(0) - v.min(0)).max())
        lo, hi = (v.min(0) - centre) * 2 / ext, (v.max(0) - centre) * 2 / ext
        assert (pts >= lo - 1e-5).all() and (pts <= hi + 1e-5).all()
        written += 1
    assert written > 0


def test_evaluate_clean_equals_cleaning_the_files_first(tmp_path):
    from octfusion_amd import evaluate as E, mesh
    raw, pre = tmp_path / 'raw', tmp_path / 'pre'
    fields = [C.two_spheres(48), C.rod_and_ball(64)]
    for k, fld in enumerate(fields):
        v, f = M.marching_cubes(fld, scale=0.5)
        mesh.write_obj(str(raw / ('%d.obj' % k)), v, f)
        cv, cf, _ = C.clean(*mesh.read_obj(str(raw / ('%d.obj' % k))))
        mesh.write_obj(str(pre / ('%d.obj' % k)), cv, cf)
    a = E.load_clouds(str(raw), points=512, seed=3, clean=True)
    b = E.load_clouds(str(pre), points=512, seed=3)
    c = E.load_clouds(str(raw), points=512, seed=3)
    assert torch.equal(a, b) and not torch.equal(a, c)
    ra = E.main(['--samples', str(raw), '--refs', str(pre), '--points', '256', '--clean', '--no-emd'])
    rb = E.main(['--samples', str(pre), '--refs', str(pre), '--points', '256', '--no-emd'])
    assert ra == rb
