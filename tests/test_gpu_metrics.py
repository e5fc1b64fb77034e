"""Evaluation metrics on the device (csrc/ofx_metrics.hip through octfusion_amd.metrics) against the float64 oracle
(tests/metrics_oracle.py): surface sampling, the Chamfer and approximate-EMD matrices, evaluate end to end, the
evaluate CLI and generate --points."""
import json
import os

import numpy as np
import pytest
import torch

import mc_oracle as MC
import metrics_oracle as O

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

KEYS = ['lgan_mmd-CD', 'lgan_cov-CD', 'lgan_mmd_smp-CD', 'lgan_mmd-EMD', 'lgan_cov-EMD', 'lgan_mmd_smp-EMD',
        '1-NN-CD-acc_t', '1-NN-CD-acc_f', '1-NN-CD-acc', '1-NN-EMD-acc_t', '1-NN-EMD-acc_f', '1-NN-EMD-acc']


def dev():
    return torch.device('cuda:0')


def mc_meshes(fields):
    from octfusion_amd import mesh
    if len({f.shape for f in fields}) > 1:
        return [m for f in fields for m in mesh.marching_cubes(torch.from_numpy(f[None]).to(dev()))]
    return mesh.marching_cubes(torch.from_numpy(np.stack(fields)).to(dev()))


def rel_err(a, b, floor=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(np.abs(b), floor)).max())


# ------------------------------------------------------------------------------------------------ sampling
@pytest.mark.parametrize('normalize', [True, False])
def test_sampling_matches_the_oracle(normalize):
    from octfusion_amd import metrics
    meshes = mc_meshes([MC.sphere(64, r=0.5), MC.torus(48), MC.gaussians(40, seed=3)])
    n, seed = 4096, 17
    pts = metrics.sample_surface(meshes, n=n, seed=seed, normalize=normalize).cpu().numpy()
    assert pts.shape == (3, n, 3) and pts.dtype == np.float32
    agree = total = 0
    for b, (v, f) in enumerate(meshes):
        v, f = v.cpu().numpy(), f.cpu().numpy()
        want, t = O.sample_surface(v, f, n, seed=seed, shape=b, normalize=normalize)
        same = np.abs(pts[b] - want).max(1) <= 1e-6
        agree += int(same.sum())
        total += n
        vv = v.astype(np.float64)
        if normalize:
            c, s = O.normalize_frame(v)
            vv = (vv - c) * s
        for k in np.nonzero(~same)[0]:         # a choice flipped at an fp CDF boundary: still on a triangle
            d = O.point_triangle_distance(np.repeat(pts[b, k][None], len(f), 0), vv[f[:, 0]], vv[f[:, 1]], vv[f[:, 2]])
            assert d.min() <= 1e-6
        if normalize:
            lo, hi = vv.min(0), vv.max(0)
            assert np.abs((lo + hi) / 2).max() < 1e-6 and abs((hi - lo).max() - 2) < 1e-5
            assert np.abs(pts[b]).max() <= 1 + 1e-5
    assert agree >= 0.999 * total, (agree, total)


def test_sampling_is_reproducible_and_keyed_by_seed_and_id():
    from octfusion_amd import metrics
    meshes = mc_meshes([MC.torus(48), MC.sphere(48)])
    a = metrics.sample_surface(meshes, n=2048, seed=5)
    b = metrics.sample_surface(meshes, n=2048, seed=5)
    c = metrics.sample_surface(meshes, n=2048, seed=6)
    assert torch.equal(a, b) and not torch.equal(a, c)
    # ids: a shape keeps its points in any batch
    d = metrics.sample_surface(meshes[1:], n=2048, seed=5, ids=[1])
    assert torch.equal(d[0], a[1])
    e = metrics.sample_surface([(v.cpu().numpy(), f.cpu().numpy()) for v, f in meshes], n=2048, seed=5)
    assert torch.equal(e, a)


def test_sampling_a_sphere_is_area_uniform():
    from octfusion_amd import metrics
    R, r, c = 128, 0.5, np.array([0.013, -0.021, 0.007])
    (m,) = mc_meshes([MC.sphere(R, r=r)])
    n = 20000
    p = metrics.sample_surface([m], n=n, seed=1, normalize=False)[0].cpu().numpy().astype(np.float64)
    d = np.linalg.norm(p - c, axis=1)
    assert np.abs(d - r).max() < 1.8 / R
    # Archimedes: equal-height zones of a sphere have equal area
    counts = np.histogram(p[:, 2] - c[2], bins=8, range=(-r, r))[0]
    expect = n / 8
    assert float(((counts - expect) ** 2 / expect).sum()) < 24.32     # chi-square, 7 dof, p = 0.001


def test_sampling_an_empty_shape_raises():
    from octfusion_amd import metrics
    meshes = mc_meshes([MC.sphere(24), np.ones((24, 24, 24), np.float32)])
    with pytest.raises(ValueError, match='shape 1'):
        metrics.sample_surface(meshes, n=16)
    v, f = meshes[0]
    with pytest.raises(ValueError, match='shape 0'):
        metrics.sample_surface([(v, f.clone().fill_(int(v.shape[0])))], n=16)


# ------------------------------------------------------------------------------------------------ Chamfer
def clouds(seed, N, n):
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1, 1, (N, 1, 3)) * 0.3
    return (rng.uniform(-1, 1, (N, n, 3)) * rng.uniform(0.2, 1.0, (N, 1, 3)) + base).astype(np.float32)


@pytest.mark.parametrize('n,NA,NB', [(1, 1, 1), (7, 1, 1), (64, 1, 1), (2048, 1, 1), (2500, 1, 1),
                                     (1, 3, 37), (7, 3, 37), (64, 3, 37), (2048, 3, 37), (2500, 3, 37),
                                     (7, 300, 300), (64, 300, 300)])
def test_chamfer_matrix_matches_the_oracle(n, NA, NB):
    from octfusion_amd import metrics
    X, Y = clouds(n * 7 + NA, NA, n), clouds(n * 11 + NB, NB, n if n < 2048 else n - 3)
    CD = metrics.chamfer_matrix(torch.from_numpy(X).to(dev()), torch.from_numpy(Y).to(dev())).cpu().numpy()
    assert rel_err(CD, O.chamfer_matrix(X, Y)) < 1e-4
    S = metrics.chamfer_matrix(torch.from_numpy(X).to(dev())).cpu().numpy()
    assert (np.diag(S) == 0).all() and np.array_equal(S, S.T)
    if NA > 1:
        assert rel_err(S, O.chamfer_matrix(X)) < 1e-4
    D = metrics.nn_matrix(torch.from_numpy(X).to(dev()), torch.from_numpy(Y).to(dev())).cpu().numpy()
    if NA * NB <= 111:
        assert rel_err(D, O.nn_matrix(X, Y)) < 1e-4


# ------------------------------------------------------------------------------------------------ EMD
@pytest.mark.parametrize('n,NA,NB', [(16, 3, 5), (128, 3, 4), (2048, 1, 2)])
def test_emd_matrix_matches_the_oracle(n, NA, NB):
    from octfusion_amd import metrics
    X, Y = clouds(n + 1, NA, n), clouds(n + 2, NB, n)
    Xd, Yd = torch.from_numpy(X).to(dev()), torch.from_numpy(Y).to(dev())
    for A, B, Ad, Bd in ((X, Y, Xd, Yd), (Y, X, Yd, Xd)):          # both orientations
        E = metrics.emd_matrix(Ad, Bd).cpu().numpy()
        assert rel_err(E, O.emd_matrix(A, B)) < 1e-3
    S = metrics.emd_matrix(Xd).cpu().numpy()
    assert np.abs(np.diag(S)).max() < 1e-5


def test_emd_rejects_unequal_and_too_large_clouds():
    from octfusion_amd import _lib, metrics
    with pytest.raises(ValueError):
        metrics.emd_matrix(torch.zeros(2, 16, 3, device=dev()), torch.zeros(2, 17, 3, device=dev()))
    with pytest.raises(ValueError):
        metrics.emd_matrix(torch.zeros(1, 2049, 3, device=dev()))
    x = torch.zeros(1, 2049, 3, device=dev())
    with pytest.raises(_lib.OfxError):
        _lib.call('ofx_emd_matrix', _lib.ptr(x), 1, _lib.ptr(x), 1, 2049, 2049, _lib.ptr(x), _lib.stream())


# ------------------------------------------------------------------------------------------------ end to end
def analytic_fields(seed, count, R=32):
    rng = np.random.default_rng(seed)
    x, y, z = MC.lattice_coords(R)
    out = []
    for k in range(count):
        c = rng.uniform(-0.2, 0.2, 3)
        if k % 3 == 0:
            f = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - rng.uniform(0.3, 0.6)
        elif k % 3 == 1:
            q = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2) - rng.uniform(0.35, 0.5)
            f = np.sqrt(q ** 2 + (z - c[2]) ** 2) - rng.uniform(0.1, 0.2)
        else:
            h = rng.uniform(0.2, 0.6, 3)
            d = np.abs(np.stack([x - c[0], y - c[1], z - c[2]])) - h[:, None, None, None]
            f = np.linalg.norm(np.maximum(d, 0), axis=0) + np.minimum(d.max(0), 0)
        out.append(f.astype(np.float32))
    return out


def test_evaluate_end_to_end_against_the_oracle():
    from octfusion_amd import metrics
    n = 128
    S = metrics.sample_surface(mc_meshes(analytic_fields(1, 48)), n=n, seed=3)
    R = metrics.sample_surface(mc_meshes(analytic_fields(2, 40)), n=n, seed=4)
    res = metrics.evaluate(S, R)
    assert list(res) == ['lgan_mmd-CD', 'lgan_cov-CD', 'lgan_mmd_smp-CD', '1-NN-CD-acc_t', '1-NN-CD-acc_f',
                         '1-NN-CD-acc', 'lgan_mmd-EMD', 'lgan_cov-EMD', 'lgan_mmd_smp-EMD', '1-NN-EMD-acc_t',
                         '1-NN-EMD-acc_f', '1-NN-EMD-acc']
    Sh, Rh = S.cpu().numpy(), R.cpu().numpy()
    want = O.evaluate(Sh, Rh)
    for k in KEYS:
        if 'mmd' in k:
            assert res[k] == pytest.approx(want[k], rel=1e-4 if 'CD' in k else 1e-3), k
    # the discrete metrics exactly, with the oracle's reductions fed the device matrices
    t = len(Rh)
    CD = metrics.chamfer_matrix(torch.cat([R, S])).cpu().numpy()
    E_ru = metrics.emd_matrix(R, torch.cat([R, S])).cpu().numpy()
    E_ss = metrics.emd_matrix(S[:t]).cpu().numpy()
    nr = len(Rh)
    got = O.cov_mmd_from(CD[:nr, nr:], E_ru[:, nr:])
    got.update(O.one_nna_from(CD[:nr, :nr], CD[:nr, nr:nr + t], CD[nr:nr + t, nr:nr + t], E_ru[:, :nr],
                              E_ru[:, nr:nr + t], E_ss))
    for k in KEYS:
        if 'cov' in k or 'acc' in k:
            assert res[k] == got[k], k
        else:
            assert res[k] == pytest.approx(got[k], rel=1e-12), k
    # cov_mmd / one_nna alone give the same numbers (one_nna over all samples)
    cm = metrics.cov_mmd(S, R)
    assert all(cm[k] == pytest.approx(res[k], rel=1e-6) for k in cm)
    nna = metrics.one_nna(S[:t], R)
    assert all(nna[k] == res[k] for k in nna)


def test_evaluate_cli(tmp_path, capsys):
    from octfusion_amd import evaluate, mesh, metrics
    meshes = mc_meshes(analytic_fields(5, 6))
    sd = tmp_path / 'samples'
    for i, (v, f) in enumerate(meshes):
        assert mesh.write_obj(str(sd / ('%d.obj' % i)), v, f)
    refs = metrics.sample_surface(mc_meshes(analytic_fields(6, 5)), n=256, seed=9).cpu()
    rd = tmp_path / 'refs'
    rd.mkdir()
    for i in range(len(refs)):
        np.save(str(rd / ('%d.npy' % i)), refs[i].numpy())
    torch.save(refs, str(tmp_path / 'refs.pt'))
    out = []
    for r in (str(rd), str(tmp_path / 'refs.pt')):
        p = str(tmp_path / 'm.json')
        res = evaluate.main(['--samples', str(sd), '--refs', r, '--points', '256', '--seed', '2', '--out', p])
        line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1]
        assert json.loads(line) == res == json.load(open(p))
        assert sorted(res) == sorted(KEYS)
        out.append(res)
    assert out[0] == out[1]
    res = evaluate.main(['--samples', str(sd), '--refs', str(rd), '--points', '256', '--seed', '2', '--no-emd'])
    assert sorted(res) == sorted(k for k in KEYS if 'CD' in k)
    assert all(res[k] == out[0][k] for k in res)


def test_generate_cli_writes_point_clouds(tmp_path, capsys):
    from octfusion_amd import configs, generate as G, mesh, metrics
    configs.CONFIGS['tiny_uncond'] = dict(configs.SNET_UNCOND, model_channels=[32, 32])
    configs.VAES['tiny_uncond'] = configs.VAES['snet_uncond']
    mesh.MESH_SCALES['tiny_uncond'] = mesh.MESH_SCALES['snet_uncond']
    out_dir = str(tmp_path / 'gen')
    res = G.main(['--config', 'tiny_uncond', '--shapes', '3', '--steps', '4', '--batch', '2', '--sdf-resolution', '64',
                  '--seed', '5', '--mesh', '--points', '256', '--out', out_dir])
    written = 0
    for i in res['rank0_indices']:
        obj = os.path.join(out_dir, '%d.obj' % i)
        npy = os.path.join(out_dir, '%d.npy' % i)
        assert os.path.exists(npy) == os.path.exists(obj)
        if not os.path.exists(obj):
            continue
        pts = np.load(npy)
        assert pts.shape == (256, 3) and pts.dtype == np.float32
        # the OBJ round trip is exact, so sampling the written mesh with the same key gives the same points
        again = metrics.sample_surface([mesh.read_obj(obj)], n=256, seed=5, ids=[i])[0].cpu().numpy()
        assert np.array_equal(pts, again)
        written += 1
    assert written > 0
