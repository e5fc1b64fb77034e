"""GPU tests of the mesh graph, the vertex normals and the smoothing (csrc/ofx_meshsmooth.hip; mesh_smooth.adjacency /
vertex_normals / smooth, sample(mesh_smooth=), the command line) against the float64 oracle (tests/smooth_oracle.py) on
the meshes of tests/smooth_cases.py.  tests/test_smooth_oracle.py pins that oracle to hand-written answers on the CPU.

What must be equal: every integer -- row_off, nbr, vflags, corner_off, corner.
Smoothing: |out64 - oracle| <= 1e-10 x the bounding-box diagonal.  Device and oracle do the same fp64 operations in the
same order, so only last-bit differences of library functions could separate them; the oracle with its sums in a
RANDOM order moves by <= 4.5e-16 after 10 Taubin iterations on the noisy icosphere (both weights), and 1e-10 is the
margin the project gives fp64 sums elsewhere (test_gpu_meshcheck.py).  The deviation is printed.  The fp32 output is the
device's own out64 rounded, bitwise.
Normals: within 2^-23 per component of the oracle's normal rounded to fp32, at every vertex whose unnormalised sum is
at least 1e-3 of the sum of its terms' lengths (where the terms cancel, the direction is rounding noise).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import meshcheck_cases as C
import smooth_cases as SC
import smooth_oracle as SO

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-10
INTS = ('row_off', 'nbr', 'vflags', 'corner_off', 'corner')


def dev():
    return torch.device('cuda:0')


def to_dev(m):
    v, f = m
    return (torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev()),
            torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(dev()))


def diagonal(v):
    used = v[np.isfinite(v).all(axis=1)].astype(np.float64)
    return float(np.linalg.norm(used.max(axis=0) - used.min(axis=0)))


def bits(t):
    """A tensor as integers, so that equal means bitwise equal (NaN included)."""
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def smooth64(meshes, **kw):
    from octfusion_amd import mesh_smooth as MS
    return [v for v, _ in MS.smooth(meshes, dtype=torch.float64, **kw)]


@pytest.fixture(scope='module')
def meshes():
    return SC.all_meshes()


@pytest.fixture(scope='module')
def on_device(meshes):
    return [to_dev(m) for _, m in meshes]


@pytest.fixture(scope='module')
def adj_oracle(meshes):
    return {name: SO.adjacency(*m) for name, m in meshes}


# ---- 1 adjacency ----------------------------------------------------------------------------------------------------
def test_adjacency_equals_the_oracle_in_every_integer(meshes, on_device, adj_oracle):
    from octfusion_amd import mesh_smooth as MS
    res = MS.adjacency(on_device, corners=True)
    assert len(res) == len(meshes)
    for (name, (v, f)), r in zip(meshes, res):
        got = dict(zip(INTS, (r[0], r[1], r[2], r[3], r[4])))
        for k in INTS:
            have, want = got[k].cpu().numpy().astype(np.int64), adj_oracle[name][k]
            assert have.shape == want.shape and np.array_equal(have, want), (name, k)
        print(name, len(v), 'vertices', len(f), 'faces', len(adj_oracle[name]['nbr']), 'neighbours, longest row',
              int(np.diff(adj_oracle[name]['row_off']).max()))
    by = dict(zip([n for n, _ in meshes], res))
    assert int(np.diff(adj_oracle['fan1000']['row_off']).max()) == 1000
    assert by['cube'][2].tolist() == [1] * 8 and by['removed'][2].tolist() == [1, 1, 3, 1, 1, 1, 3, 3]
    assert by['defects'][2].tolist()[8:] == [3, 0, 0] and (by['random_signs'][2] & 4).any()
    plain = MS.adjacency(on_device[:3])                    # without the corner lists: the same rows
    for a, b in zip(plain, res[:3]):
        assert len(a) == 3 and all(same(x, y) for x, y in zip(a, b[:3]))


# ---- 2 smoothing ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('weights', ['uniform', 'cot'])
@pytest.mark.parametrize('boundary', ['fixed', 'slide', 'free'])
@pytest.mark.parametrize('mu', [None, -0.53], ids=['laplacian', 'taubin'])
def test_smooth_equals_the_oracle(meshes, on_device, weights, boundary, mu):
    from octfusion_amd import mesh_smooth as MS
    worst = 0.0
    for iters in (1, 2, 10):
        kw = dict(iterations=iters, lam=0.5, mu=mu, weights=weights, boundary=boundary)
        out64 = smooth64(on_device, **kw)
        out32 = MS.smooth(on_device, **kw)
        for (name, (v, f)), o64, (o32, faces), m in zip(meshes, out64, out32, on_device):
            want = SO.smooth(v, f, iters, 0.5, mu, SO.WEIGHTS[weights], SO.BOUNDARY[boundary])
            have = o64.cpu().numpy()
            used = (SO.adjacency(v, f)['vflags'] & 1) > 0
            err = np.abs(have[used] - want[used]).max() / diagonal(v)
            worst = max(worst, err)
            assert err <= BOUND, (name, iters, err)
            assert np.array_equal(have[~used].view(np.int64), v[~used].astype(np.float64).view(np.int64)), name
            assert faces is m[1] and o32.dtype == torch.float32
            rounded = o64.to(torch.float32)
            moved = torch.from_numpy(used).to(dev())
            assert same(o32[moved], rounded[moved]), (name, iters)
            assert same(o32[~moved], m[0][~moved]), (name, iters)
    print('%s / %s / %s: the largest |device - oracle| is %.3e of the bounding-box diagonal'
          % (weights, boundary, 'laplacian' if mu is None else 'taubin', worst))


# ---- 3 vertex normals -----------------------------------------------------------------------------------------------
def test_vertex_normals_equal_the_oracle(meshes, on_device):
    from octfusion_amd import mesh_smooth as MS
    cancelling = set()
    for weight, mode in SO.MODES.items():
        res = MS.vertex_normals(on_device, weight=weight)
        worst = 0.0
        for (name, (v, f)), n in zip(meshes, res):
            if name == 'flipped':                          # its normals are what the flipped face makes of them
                continue
            want, s, lengths = SO.vertex_normals(v, f, mode)
            sound = np.sqrt((s * s).sum(axis=1)) >= 1e-3 * lengths
            if not sound.all():
                cancelling.add(name)
            have = n.cpu().numpy()
            assert have.dtype == np.float32 and have.shape == v.shape
            err = np.abs(have[sound].astype(np.float64) - want[sound].astype(np.float32).astype(np.float64)).max()
            worst = max(worst, err)
            assert err <= 2.0 ** -23, (name, weight, err)
            unused = (SO.adjacency(v, f)['vflags'] & 1) == 0
            assert (have[unused] == 0).all(), name
        print('%s: the largest |device - oracle| component is %.3e = %.2f x 2^-23' % (weight, worst, worst * 2 ** 23))
    # terms cancel only where the simplified torus has folded two faces onto each other
    assert cancelling == {'simplified_torus'}, cancelling
    cube = MS.vertex_normals([to_dev(C.cube(2.0))], weight='angle')[0].cpu().numpy().astype(np.float64)
    assert np.abs(cube - (C.cube(2.0)[0].astype(np.float64) - 1.0) / np.sqrt(3.0)).max() <= 2.0 ** -23


# ---- 4 purity -------------------------------------------------------------------------------------------------------
def everything(ms):
    """Every output of the three entries on a batch, per mesh, as a flat list of tensors."""
    from octfusion_amd import mesh_smooth as MS
    adj = MS.adjacency(ms, corners=True)
    nrm = MS.vertex_normals(ms, weight='angle')
    uni = smooth64(ms, iterations=3)
    cot = smooth64(ms, iterations=3, weights='cot', boundary='slide')
    f32 = MS.smooth(ms, iterations=3, mu=None, boundary='free')
    return [list(a) + [n, u, c, s[0]] for a, n, u, c, s in zip(adj, nrm, uni, cot, f32)]


def test_batch_order_and_run_do_not_change_a_bit(meshes, on_device):
    names = [n for n, _ in meshes]
    pick = [names.index('icosphere'), names.index('removed'), names.index('defects')]
    three = [on_device[k] for k in pick]
    base = everything(three)
    for k, m in enumerate(three):
        alone = everything([m])[0]
        assert all(same(a, b) for a, b in zip(alone, base[k])), names[pick[k]]
    for a, b in zip(everything(three[::-1])[::-1], base):
        assert all(same(x, y) for x, y in zip(a, b))
    tetra = to_dev(SC.TETRA)
    many = everything([tetra] * 150 + [three[0]] + [tetra] * 149)
    assert all(same(x, y) for x, y in zip(many[150], base[0]))
    assert all(all(same(x, y) for x, y in zip(many[k], many[0])) for k in (1, 149, 151, 299))
    for a, b in zip(everything(three), base):                                # a second run
        assert all(same(x, y) for x, y in zip(a, b))


def test_a_permutation_of_the_faces(meshes):
    v, f = dict(meshes)['icosphere']
    perm = np.random.default_rng(5).permutation(len(f))
    a, b = to_dev((v, f)), to_dev((v, f[perm]))
    kw = dict(iterations=10, lam=0.5, mu=-0.53)
    assert same(smooth64([a], **kw)[0], smooth64([b], **kw)[0])              # uniform: the rows are the same sets
    ca, cb = smooth64([a], weights='cot', **kw)[0], smooth64([b], weights='cot', **kw)[0]
    err = float((ca - cb).abs().max()) / diagonal(v)
    print('cotangent weights, faces permuted: moved by %.3e of the diagonal' % err)
    assert err <= BOUND


# ---- 5 edge cases ---------------------------------------------------------------------------------------------------
def test_edge_cases(meshes):
    from octfusion_amd import mesh_smooth as MS
    by = dict(meshes)
    d = to_dev(by['defects'])
    for dtype in (torch.float32, torch.float64):
        out = MS.smooth([d, to_dev(by['icosphere'])], iterations=0, dtype=dtype)
        assert same(out[0][0], d[0].to(dtype)) and same(out[1][0], to_dev(by['icosphere'])[0].to(dtype))
    out = MS.smooth([d], iterations=10, boundary='free')[0][0]
    assert same(out[9:], d[0][9:]) and torch.isnan(out[10]).all() and not same(out[:8], d[0][:8])
    nrm = MS.vertex_normals([d])[0]
    assert (nrm[8:] == 0).all() and (nrm[:8].norm(dim=1) - 1).abs().max() < 1e-6
    hole = to_dev(by['removed'])
    for weights in ('uniform', 'cot'):
        fixed = MS.smooth([hole], iterations=10, weights=weights, boundary='fixed')[0][0]
        assert same(fixed[[2, 6, 7]], hole[0][[2, 6, 7]]) and not same(fixed, hole[0])
        slide = MS.smooth([hole], iterations=10, weights=weights, boundary='slide')[0][0]
        assert (slide[[2, 6, 7], 1] == 2.0).all() and not same(slide[[2, 6, 7]], hole[0][[2, 6, 7]])
    rim = MS.smooth([to_dev(by['fan1000'])], iterations=2)[0][0]
    assert same(rim[1:], to_dev(by['fan1000'])[0][1:]) and not same(rim[:1], to_dev(by['fan1000'])[0][:1])


# ---- 6 refusals -----------------------------------------------------------------------------------------------------
def test_bad_meshes_and_arguments_are_refused():
    from octfusion_amd import mesh_smooth as MS
    good = [to_dev(C.cube(2.0)), to_dev(C.strip(7))]
    v, f = C.cube(2.0)
    bad_index = to_dev((v, np.concatenate([f, [[0, 1, 8]]]).astype(np.int32)))
    nan_used = to_dev((np.where(np.arange(8)[:, None] == 5, np.float32('nan'), v).astype(np.float32), f))
    for bad in (bad_index, nan_used):
        for fn in (MS.smooth, MS.adjacency, MS.vertex_normals):
            with pytest.raises(ValueError, match='shape 1 '):
                fn([good[0], bad, good[1]])
            with pytest.raises(ValueError, match='shape 0 '):
                fn([bad])
    launches = []
    from octfusion_amd import _lib
    real = _lib.call
    _lib.call = MS.call = lambda *a: launches.append(a)
    try:
        for kw in (dict(lam=0.0), dict(lam=1.5), dict(lam=float('nan')), dict(mu=0.1), dict(mu=0.0),
                   dict(mu=float('-inf')), dict(iterations=-1), dict(iterations=10001), dict(weights='cotan'),
                   dict(boundary='pinned'), dict(dtype=torch.float16)):
            with pytest.raises(ValueError):
                MS.smooth(good, **kw)
        with pytest.raises(ValueError):
            MS.vertex_normals(good, weight='face')
    finally:
        _lib.call = MS.call = real
    assert not launches


def test_entry_points_refuse_bad_arguments():
    from octfusion_amd import _lib
    L = _lib.lib()
    assert L.ofx_mesh_adjacency_ws_bytes(0, 8, 12) == 0 and L.ofx_mesh_adjacency_ws_bytes(65536, 8, 12) == 0
    assert L.ofx_mesh_adjacency_ws_bytes(1, 2 ** 30 + 1, 12) == 0 and L.ofx_mesh_smooth_ws_bytes(1, 8, 0, 0) == 0
    assert L.ofx_mesh_vertex_normals_ws_bytes(1, 8, 2 ** 30 // 6 + 1) == 0 and L.ofx_mesh_smooth_ws_bytes(1, 8, 12, 2) == 0
    assert L.ofx_mesh_adjacency_ws_bytes(1, 8, 12) > 0 and L.ofx_mesh_vertex_normals_ws_bytes(1, 8, 12) > 0
    assert L.ofx_mesh_smooth_ws_bytes(1, 8, 12, 1) > L.ofx_mesh_smooth_ws_bytes(1, 8, 12, 0) > 0
    v, f = to_dev(C.cube(2.0))
    offs = torch.tensor([[0, 8], [0, 12]], dtype=torch.int64, device=dev())
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev())
    sentinel = torch.full((256,), -77, dtype=torch.int32, device=dev())
    s = sentinel.clone()
    p = _lib.ptr
    mesh_args = (p(v), p(f), p(offs[0]), p(offs[1]))
    smooth = lambda batch, iters, out, weights=0, boundary=0, lam=0.5: L.ofx_mesh_smooth(
        *mesh_args, batch, 8, 12, weights, boundary, lam, -0.53, iters, out, None, p(ws), p(s), None)
    assert smooth(1, 1, None) == -1 and smooth(0, 1, p(s)) == -1 and smooth(65536, 1, p(s)) == -1
    assert smooth(1, -1, p(s)) == -1 and smooth(1, 10001, p(s)) == -1 and smooth(1, 1, p(s), weights=2) == -1
    assert smooth(1, 1, p(s), boundary=3) == -1 and smooth(1, 1, p(s), lam=float('nan')) == -1
    adj = lambda batch, row_off, corner: L.ofx_mesh_adjacency(*mesh_args, batch, 8, 12, row_off, p(s), p(s), p(s),
                                                              corner, p(ws), p(s), None)
    assert adj(1, None, p(s)) == -1 and adj(0, p(s), p(s)) == -1 and adj(65536, p(s), p(s)) == -1
    assert adj(1, p(s), None) == -1                        # one of the two corner arrays alone
    nrm = lambda batch, mode, out: L.ofx_mesh_vertex_normals(*mesh_args, batch, 8, 12, mode, out, p(ws), p(s), None)
    assert nrm(1, 1, None) == -1 and nrm(0, 1, p(s)) == -1 and nrm(1, 3, p(s)) == -1 and nrm(1, -1, p(s)) == -1
    torch.cuda.synchronize()
    assert torch.equal(s, sentinel)


# ---- 7 what smoothing is for ----------------------------------------------------------------------------------------
def test_taubin_removes_the_noise_and_keeps_the_volume_laplacian_shrinks(meshes):
    from octfusion_amd import mesh_check as MC, mesh_smooth as MS
    m = to_dev(dict(meshes)['icosphere'])
    taubin = MS.smooth([m], iterations=10, lam=0.5, mu=-0.53)[0]
    laplace = MS.smooth([m], iterations=10, lam=0.5, mu=None)[0]
    vol = [r['volume'] for r in MC.check([m, taubin, laplace], weld=False, intersections=False)]
    radial = [float(x[0].double().norm(dim=1).std(unbiased=False)) for x in (m, taubin)]
    print('radial deviation %.4f -> %.4f; volume x %.4f (Taubin), x %.4f (Laplacian)'
          % (radial[0], radial[1], vol[1] / vol[0], vol[2] / vol[0]))
    assert radial[1] < 0.5 * radial[0]
    assert abs(vol[1] / vol[0] - 1.0) < 0.05
    assert vol[2] / vol[0] < 0.7


# ---- 8 the pipeline -------------------------------------------------------------------------------------------------
def test_marching_cubes_then_smooth_stays_watertight():
    from octfusion_amd import mesh, mesh_check as MC, mesh_smooth as MS
    sdf = torch.from_numpy(SC.ripple_lattice(32)).to(dev())[None]
    raw = mesh.marching_cubes(sdf)[0]
    assert raw[1].shape[0] > 1000
    out = MS.smooth([raw], iterations=5)[0]
    assert out[1] is raw[1] and out[0].shape == raw[0].shape and not same(out[0], raw[0])
    before, after = MC.check([raw, out], weld=False)
    assert before['watertight'] and before['oriented'] and after['watertight'] and after['oriented']
    assert after['euler'] == before['euler'] == 2
    v, f = raw[0].cpu().numpy(), raw[1].cpu().numpy()
    want = SO.smooth(v, f, 5)
    err = np.abs(smooth64([raw], iterations=5)[0].cpu().numpy() - want).max() / diagonal(v)
    print('%d faces: |device - oracle| = %.3e of the diagonal' % (len(f), err))
    assert err <= BOUND


# ---- 9 the command line ---------------------------------------------------------------------------------------------
def test_mesh_smooth_command_line(tmp_path, meshes):
    from octfusion_amd import mesh, mesh_smooth as MS
    by = dict(meshes)
    a, b = str(tmp_path / 'ico.obj'), str(tmp_path / 'removed.obj')
    mesh.write_obj(a, *by['icosphere'])
    mesh.write_obj(b, *by['removed'])
    out_dir = str(tmp_path / 'out')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    run = subprocess.run([sys.executable, '-m', 'octfusion_amd.mesh_smooth', '--input', a, b, '--out', out_dir,
                          '--iterations', '3', '--boundary', 'slide', '--normals'], capture_output=True, text=True,
                         cwd=ROOT, env=env)
    assert run.returncode == 0, run.stderr[-2000:]
    rows = [json.loads(l) for l in run.stdout.splitlines() if l.startswith('{')]
    assert [r['vertices'] for r in rows] == [162, 8] and [r['faces'] for r in rows] == [320, 11]
    for src, row in zip((a, b), rows):
        v0, f0 = mesh.read_obj(src)
        v, f = mesh.read_obj(row['out'])
        assert v.shape == v0.shape and np.array_equal(f, f0)
        want = MS.smooth([to_dev((v0, f0))], iterations=3, boundary='slide')[0][0]
        assert np.array_equal(v.view(np.uint32), want.cpu().numpy().view(np.uint32))
        nrm = MS.vertex_normals([to_dev((v, f))])[0].cpu().numpy().astype(np.float64)
        vn = [l for l in open(row['out']).read().splitlines() if l.startswith('vn ')]
        assert vn == ['vn %.9g %.9g %.9g' % tuple(r) for r in nrm.tolist()]


GENERATE = """
import sys
from octfusion_amd import configs, generate, mesh
configs.CONFIGS['tiny_uncond'] = dict(configs.SNET_UNCOND, model_channels=[32, 32])
configs.VAES['tiny_uncond'] = configs.VAES['snet_uncond']
mesh.MESH_SCALES['tiny_uncond'] = mesh.MESH_SCALES['snet_uncond']
generate.main(['--config', 'tiny_uncond', '--shapes', '1', '--steps', '2', '--batch', '1', '--sdf-resolution', '32',
               '--seed', '5', '--mesh', '--out', sys.argv[1]] + sys.argv[2:])
"""


def test_generate_command_line_writes_the_smoothed_mesh(tmp_path):
    from octfusion_amd import mesh, mesh_smooth as MS
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    plain, smooth = str(tmp_path / 'plain'), str(tmp_path / 'smooth')
    lines = []
    for out, more in ((plain, []), (smooth, ['--smooth', '3', '--smooth-normals', '--check'])):
        run = subprocess.run([sys.executable, '-c', GENERATE, out] + more, capture_output=True, text=True, cwd=ROOT,
                             env=env)
        assert run.returncode == 0, run.stderr[-2000:]
        lines.append([json.loads(l) for l in run.stdout.splitlines() if l.startswith('{')][-1])
    assert lines[0]['rank0_mesh_faces'] == lines[1]['rank0_mesh_faces']
    if not lines[0]['rank0_mesh_faces'][0]:
        return                                             # the random weights gave an empty mesh: nothing is written
    v0, f0 = mesh.read_obj(os.path.join(plain, '0.obj'))
    v, f = mesh.read_obj(os.path.join(smooth, '0.obj'))
    assert np.array_equal(f, f0) and v.shape == v0.shape
    want = MS.smooth([to_dev((v0, f0))], iterations=3)[0][0].cpu().numpy()
    assert np.array_equal(v.view(np.uint32), want.view(np.uint32))
    text = open(os.path.join(smooth, '0.obj')).read().splitlines()
    assert sum(l.startswith('vn ') for l in text) == len(v)
    assert not any(l.startswith('vn ') for l in open(os.path.join(plain, '0.obj')).read().splitlines())
    assert lines[1]['rank0_mesh_check'][0]['faces'] == len(f)
