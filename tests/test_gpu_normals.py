"""GPU checks of octfusion_amd.normals (csrc/ofx_normals.hip) against tests/normals_oracle.py, and of
``reconstruct --estimate-normals``.

kNN        idx equal and d2 bit-equal to the oracle's full sort, for k in {1, 16, 33, 64} and cells in {0, 1, 2, 7}
           (cells = 1 is the brute-force sweep), alone and in a ragged batch, and on a repeat.
PCA        fed the GPU's own idx.  |dot| >= 1 - 1e-6 wherever (l1 - l0) / l2 >= 1e-3: fp32 rounding of a unit vector
           (3 components x 2^-24, and the fp64 eigenvector error at that gap is about 1e-13); variation within 4 fp32
           ulp or 1e-12 absolute.
orient     fed the GPU's unoriented normals, its idx and the cube and G it reports: the final signs, the oriented
           normals and the four counts equal the oracle's exactly.
Collinear neighbours are NOT degenerate by the contract (the eigenvalue sum is positive): the test asserts a unit normal
across the line and a variation below 1e-12; identical points and fewer than 3 neighbours are, and are counted."""
import json
import os

import numpy as np
import pytest
import torch

import normals_oracle as O
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

KS = (1, 16, 33, 64)
CELLS = (0, 1, 2, 7)


def _duplicates():
    p = O.torus(400, seed=4)[0]
    p[100:140] = p[:40]                       # exact duplicates with a higher index than their originals
    p[399] = p[200]
    return p


CLOUDS = {
    'torus_1500': lambda: O.torus(1500, seed=1)[0],
    'duplicates': _duplicates,
    'identical': lambda: np.tile(np.array([[0.25, -0.5, 0.125]], np.float32), (70, 1)),
    'lattice_300': lambda: O.lattice(300, seed=2),
    'five': lambda: O.sphere(5, seed=6)[0],
    'one': lambda: O.sphere(1, seed=7)[0],
    'ragged_700': lambda: O.box(700, seed=8)[0],
}
_cache = {}


def cloud(name):
    """(points, oracle idx [n, 64], oracle d2 [n, 64]): computed once, sliced for smaller k."""
    if name not in _cache:
        p = CLOUDS[name]()
        _cache[name] = (p,) + O.knn(p, 64)
    return _cache[name]


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def same(a, b):
    """Bitwise equality of two tensors / arrays of the same dtype (+inf and -1 included)."""
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    b = b.cpu().numpy() if torch.is_tensor(b) else b
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------ kNN
@pytest.mark.parametrize('name', ['torus_1500', 'duplicates', 'identical', 'lattice_300', 'five'])
def test_knn_vs_oracle(name):
    from octfusion_amd import normals
    p, oi, od = cloud(name)
    n = p.shape[0]
    for k in KS:
        want_i, want_d = np.ascontiguousarray(oi[:, :k]), np.ascontiguousarray(od[:, :k])
        for cells in CELLS:
            idx, d2 = normals.knn(t(p), k, cells=cells)
            assert idx.shape == d2.shape == (n, k) and idx.dtype == torch.int32 and d2.dtype == torch.float32
            assert same(idx, want_i), (name, k, cells)
            assert same(d2, want_d), (name, k, cells)
        again = normals.knn(t(p), k)
        assert same(again[0], want_i) and same(again[1], want_d)
    if name == 'duplicates':                  # the duplicate with the lower index precedes the point itself
        assert oi[100, 0] == 0 and oi[100, 1] == 100 and od[100, 1] == 0
    if name == 'five':
        assert (oi[:, 5:] == -1).all() and np.isinf(od[:, 5:]).all()


def test_knn_ragged_batch_equals_alone():
    from octfusion_amd import normals
    names = ['one', 'ragged_700', 'torus_1500']
    empty = torch.zeros(0, 3, device=dev())
    for k in (1, 16, 64):
        for cells in CELLS:
            batch = [empty, t(cloud('one')[0]), t(cloud('ragged_700')[0]), t(cloud('torus_1500')[0])]
            idx, d2 = normals.knn(batch, k, cells=cells)
            assert idx[0].shape == (0, k) and d2[0].shape == (0, k)
            for j, name in enumerate(names):
                p, oi, od = cloud(name)
                assert same(idx[j + 1], np.ascontiguousarray(oi[:, :k])), (name, k, cells)
                assert same(d2[j + 1], np.ascontiguousarray(od[:, :k])), (name, k, cells)
                alone = normals.knn(t(p), k, cells=cells)
                assert same(alone[0], idx[j + 1]) and same(alone[1], d2[j + 1])
    idx, d2 = normals.knn([empty], 4)
    assert idx[0].shape == (0, 4)


def test_knn_arguments():
    from octfusion_amd import _lib, normals
    p = t(cloud('five')[0])
    with pytest.raises(_lib.OfxError):
        normals.knn(p.cpu(), 4)
    with pytest.raises(_lib.OfxError):
        normals.estimate_normals([p, p.cpu()])
    for k in (0, 65):
        with pytest.raises(ValueError):
            normals.knn(p, k)
    L = _lib.lib()
    off = torch.tensor([0, 5], dtype=torch.int64, device=dev())
    ws = torch.zeros(int(L.ofx_knn_ws_bytes(1, 5, 5, 0)), dtype=torch.uint8, device=dev())
    idx = torch.full((5, 4), 7, dtype=torch.int32, device=dev())
    d2 = torch.full((5, 4), 7.0, device=dev())
    a = (p.data_ptr(), off.data_ptr(), 1, 5, 5, 4, 0, ws.data_ptr(), idx.data_ptr(), d2.data_ptr(), None)
    for pos, bad in ((0, None), (1, None), (7, None), (8, None), (9, None), (5, 0), (5, 65), (6, -1), (6, 129),
                     (4, 0), (4, 6), (2, -1), (3, -1)):
        b = list(a)
        b[pos] = bad
        assert L.ofx_knn(*b) == -1, (pos, bad)
    assert L.ofx_knn_ws_bytes(1, 5, 5, 129) == 0 and L.ofx_knn_ws_bytes(0, 5, 5, 0) == 0
    b = list(a)
    b[2] = 0
    assert L.ofx_knn(*b) == 0
    b = list(a)
    b[3] = 0
    assert L.ofx_knn(*b) == 0
    torch.cuda.synchronize()
    assert (idx == 7).all() and (d2 == 7).all()            # nothing was launched by any of these
    assert [L.ofx_knn_cells(n) for n in (0, 1, 127, 128, 100000, 10 ** 7)] == [1, 1, 1, 2, 55, 64]


# ------------------------------------------------------------------------------------------------------------ PCA
def gpu_pca(p, idx):
    from octfusion_amd import _lib
    n, k = idx.shape
    p, idx = t(p), t(idx.astype(np.int32))
    off = torch.tensor([0, n], dtype=torch.int64, device=dev())
    nrm = torch.empty(n, 3, device=dev())
    var = torch.empty(n, device=dev())
    deg = torch.full((1,), 99, dtype=torch.int32, device=dev())
    _lib.call('ofx_pca_normals', p.data_ptr(), off.data_ptr(), idx.data_ptr(), 1, n, n, k, nrm.data_ptr(),
              var.data_ptr(), deg.data_ptr(), _lib.stream())
    return nrm.cpu().numpy(), var.cpu().numpy(), int(deg.item())


def check_pca(p, idx):
    nrm, var, deg = gpu_pca(p, idx)
    want_n, want_v, want_deg, gap = O.pca(p, idx)
    assert deg == int(want_deg.sum())
    assert (nrm[want_deg] == 0).all() and (var[want_deg] == 0).all()
    ok = ~want_deg
    dots = (nrm.astype(np.float64) * want_n).sum(1)
    sure = ok & (gap >= 1e-3)
    assert np.abs(dots[sure]).min() >= 1 - 1e-6 if sure.any() else True
    assert np.abs(np.linalg.norm(nrm[ok].astype(np.float64), axis=1) - 1).max() <= 1e-6 if ok.any() else True
    err = np.abs(var.astype(np.float64) - want_v.astype(np.float64))
    assert (err <= np.maximum(4 * np.spacing(want_v).astype(np.float64), 1e-12)).all()
    lead = np.abs(nrm).argmax(1)                                  # the sign convention, on the output itself
    assert (nrm[np.arange(len(nrm)), lead][ok] > 0).all()
    return nrm, var, sure


@pytest.mark.parametrize('k', [3, 16, 64])
def test_pca_vs_oracle(k):
    from octfusion_amd import normals
    for name in ('torus_1500', 'lattice_300', 'duplicates'):
        p = cloud(name)[0]
        idx = normals.knn(t(p), k)[0].cpu().numpy()
        nrm, var, sure = check_pca(p, idx)
        if name == 'torus_1500' and k >= 16:
            assert sure.mean() > 0.9
        # equal up to fp32 rounding and, where two components tie for the largest within an ulp, the overall sign
        w = O.pca(p, idx)[0][sure]
        assert np.minimum(np.abs(nrm[sure] - w).max(1), np.abs(nrm[sure] + w).max(1)).max() <= 2e-6
    un, var2 = normals.estimate_normals(t(cloud('torus_1500')[0]), k=k, orient=False, return_variation=True)
    idx = normals.knn(t(cloud('torus_1500')[0]), k)[0].cpu().numpy()
    a, b, _ = gpu_pca(cloud('torus_1500')[0], idx)
    assert same(un, a) and same(var2, b)                           # the module is the entry point, bit for bit


def test_pca_degenerate_inputs():
    from octfusion_amd import normals
    line = (np.arange(40)[:, None] * np.array([[0.03, -0.02, 0.01]]) + 0.1).astype(np.float32)
    idx = normals.knn(t(line), 8)[0].cpu().numpy()
    nrm, var, deg = gpu_pca(line, idx)
    assert deg == 0                                                # collinear: sum of eigenvalues > 0, see the docstring
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1).max() <= 1e-6
    assert np.abs(nrm.astype(np.float64) @ [3.0, -2.0, 1.0]).max() / np.sqrt(14.0) <= 1e-5 and var.max() <= 1e-12
    check_pca(line, idx)
    same_pts = cloud('identical')[0]
    nrm, var, deg = gpu_pca(same_pts, normals.knn(t(same_pts), 16)[0].cpu().numpy())
    assert deg == 70 and (nrm == 0).all() and (var == 0).all()
    two = cloud('five')[0][:2]
    nrm, var, deg = gpu_pca(two, normals.knn(t(two), 16)[0].cpu().numpy())        # two valid neighbours, 14 of -1
    assert deg == 2 and (nrm == 0).all() and (var == 0).all()
    five = cloud('five')[0]
    check_pca(five, normals.knn(t(five), 16)[0].cpu().numpy())                     # five valid of sixteen
    st = {}
    out = normals.estimate_normals([t(same_pts), t(two), t(five)], stats=st)
    assert st['degenerate'] == [70, 2, 0] and st['undecided'][:2] == [70, 2] and st['G'][:2] == [8, 8]
    assert (out[0] == 0).all() and (out[1] == 0).all()


# --------------------------------------------------------------------------------------------------------- orient
SHAPES = {
    'sphere_2000': lambda: O.sphere(2000),
    'torus_4000': lambda: O.torus(4000),
    'two_spheres': lambda: O.two_spheres(2000),
    'box_6000': lambda: O.box(6000),
    'chair_8000': lambda: O.chair(8000),
}
_shape = {}


def shape(name):
    """(points, analytic normals, GPU idx, GPU unoriented normals): the GPU parts once per shape."""
    from octfusion_amd import normals
    if name not in _shape:
        p, n = SHAPES[name]()
        idx = normals.knn(t(p), 16)[0].cpu().numpy()
        un = normals.estimate_normals(t(p), k=16, orient=False).cpu().numpy()
        _shape[name] = (p, n, idx, un)
    return _shape[name]


def check_orient(name, grid=None, steps=8, rounds=3):
    from octfusion_amd import normals
    p, n, idx, un = shape(name)
    st = {}
    out = normals.estimate_normals(t(p), k=16, grid=grid, steps=steps, rounds=rounds, stats=st)
    G, lo, e = st['G'][0], np.array(st['lo'][0], np.float32), np.float32(st['e'][0])
    assert G == grid if grid is not None else 8 <= G <= 128
    want, sign, counts = O.orient(p, un, idx, lo, e, G, steps, rounds)
    got = {c: st[c][0] for c in counts}
    print(name, 'G', G, got)
    assert same(st['sign'][0], sign)
    assert got == counts
    assert same(out, want)
    return out.cpu().numpy(), n, st


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_orient_vs_oracle(name):
    out, n, st = check_orient(name)
    if name == 'chair_8000':                   # thin legs: the case with undecided points and vote flips
        assert st['undecided_after_march'][0] > 0 and st['flipped_by_vote'][0] > 0
    if name in ('sphere_2000', 'torus_4000', 'two_spheres'):      # end to end against the analytic normals
        assert st['undecided'][0] == 0 and int(((out.astype(np.float64) * n).sum(1) < 0).sum()) == 0


@pytest.mark.parametrize('grid', [8, 128])
def test_orient_grid_sizes_on_the_torus(grid):
    check_orient('torus_4000', grid=grid)


def test_orient_steps_and_rounds():
    check_orient('chair_8000', steps=3, rounds=0)
    check_orient('chair_8000', steps=1, rounds=5)


def test_orient_batch_equals_alone():
    from octfusion_amd import normals
    names = ['chair_8000', 'sphere_2000', 'torus_4000']
    sb = {}
    outs, var = normals.estimate_normals([t(shape(m)[0]) for m in names], stats=sb, return_variation=True)
    for j, m in enumerate(names):
        sa = {}
        out, v = normals.estimate_normals(t(shape(m)[0]), stats=sa, return_variation=True)
        assert same(out, outs[j]) and same(v, var[j]) and same(sa['sign'][0], sb['sign'][j])
        for key in ('G', 'lo', 'e') + normals.COUNTS:
            assert sa[key][0] == sb[key][j], (m, key)
    again = normals.estimate_normals([t(shape(m)[0]) for m in names])
    assert all(same(a, b) for a, b in zip(again, outs))


def test_points_input_and_cli(tmp_path):
    from octfusion_amd import mesh, normals
    from octfusion_amd.octree import Points
    p, n = shape('sphere_2000')[:2]
    a = normals.estimate_normals(Points(t(p)))
    assert same(a, normals.estimate_normals(t(p)))
    np.save(str(tmp_path / 'ball.npy'), p)
    mesh.write_ply(str(tmp_path / 'cloud.ply'), p[:1500])
    normals.main(['--input', str(tmp_path / 'ball.npy'), str(tmp_path / 'cloud.ply'), '--out', str(tmp_path / 'o')])
    with np.load(str(tmp_path / 'o' / 'ball' / 'pointcloud.npz')) as z:
        assert np.array_equal(z['points'], p) and same(a, z['normals'])
    q, m = mesh.read_ply(str(tmp_path / 'o' / 'cloud' / 'input.ply'))
    assert np.array_equal(q, p[:1500]) and int(((m.astype(np.float64) * n[:1500]).sum(1) < 0).sum()) == 0


# ---------------------------------------------------------------------------------------------------- reconstruct
def test_reconstruct_estimate_normals(golden, tmp_path):
    from octfusion_amd import configs, mesh, reconstruct as R, synthetic
    from octfusion_amd.graph_vae import GraphVAE
    kw = dict(golden('g_vae_enc')['cfg'])
    ps = 0.5
    p, n = O.sphere(4000, seed=9)
    raw, full = tmp_path / 'data' / 'raw', tmp_path / 'data' / 'full'
    raw.mkdir(parents=True)
    full.mkdir(parents=True)
    np.savez(str(raw / 'pointcloud.npz'), points=p * np.float32(ps))
    np.savez(str(full / 'pointcloud.npz'), points=p * np.float32(ps), normals=n)
    # ---- without the flag a cloud without normals is refused as it always was
    with pytest.raises(KeyError):
        R.read_inputs([str(raw)])
    # ---- with it, through the command line
    configs.CONFIGS['tiny_recon'] = configs.CONFIGS['snet_uncond']
    configs.VAES['tiny_recon'] = kw
    mesh.MESH_SCALES['tiny_recon'] = ps
    try:
        out = str(tmp_path / 'recon')
        res = R.main(['--config', 'tiny_recon', '--input', str(raw), '--out', out, '--estimate-normals',
                      '--sdf-resolution', '32', '--chamfer-points', '2048', '--seed', '4'])
    finally:
        del configs.CONFIGS['tiny_recon'], configs.VAES['tiny_recon'], mesh.MESH_SCALES['tiny_recon']
    saved = json.load(open(os.path.join(out, 'metrics.json')))
    rec = saved['shapes']['raw']
    assert rec['normals']['undecided'] == 0 and rec['normals']['degenerate'] == 0 and rec['normals']['k'] == 16
    assert 8 <= rec['normals']['G'] <= 128 and res['shapes']['raw']['normals'] == rec['normals']
    assert rec['faces'] > 0 and os.path.exists(os.path.join(out, 'raw', '0.obj'))
    q, m = mesh.read_ply(os.path.join(out, 'raw', 'input.ply'))
    assert len(q) == 4000 and int(((m.astype(np.float64) * n).sum(1) < 0).sum()) == 0
    # ---- an input that has normals: byte-identical files with and without the flag
    vae = GraphVAE(**kw)
    vae.load_state_dict(synthetic.random_state_dict(vae))
    vae = vae.to(dev()).eval()
    cfg = {'depth': kw['depth'], 'full_depth': kw['full_depth'], 'point_scale': ps}
    blobs = []
    for flag in (False, True):
        inputs = R.read_inputs([str(full)], estimate_normals=flag)
        d = str(tmp_path / ('with' if flag else 'without'))
        R.reconstruct(vae, cfg, inputs, dev(), sdf_resolution=32, seed=4, chamfer_points=2048, out_dir=d,
                      estimate_normals=flag)
        files = sorted(os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs)
        assert [os.path.relpath(f, d) for f in files] == ['full/0.obj', 'full/input.ply', 'metrics.json'] or \
            [os.path.relpath(f, d) for f in files] == ['full/input.ply', 'metrics.json']
        blobs.append([open(f, 'rb').read() for f in files])
    assert blobs[0] == blobs[1]
    assert 'normals' not in json.loads(blobs[0][-1])['shapes']['full']
    # ---- the function refuses a cloud without normals when the flag is off
    inputs = R.read_inputs([str(raw)], estimate_normals=True)
    with pytest.raises(ValueError):
        R.reconstruct(vae, cfg, inputs, dev(), sdf_resolution=32, chamfer_points=0)
