"""GPU checks of the reconstruction path (octfusion_amd.reconstruct): the oriented surface sampler through the C ABI
against the float64 oracle (tests/recon_oracle.py), the reference-named entry points GraphVAE.extract_code / forward
against the reference's recorded runs (g_vae_enc.pt, g_vae_train.pt) and against the hand compositions they stand for,
QKVAttention.forward against its formula, and the driver end to end on a tiny VAE with seeded random weights.

Tolerances.  Sampler normals 1e-5 absolute on triangles whose smallest angle is >= 10 degrees: an fp32 cross product
and normalisation is a few ulp times the cross product's condition 1 / sin 10deg ~ 6, and 1e-5 leaves more than tenfold
room (the kernel works in fp64 and rounds once, which is inside it); unit length 1e-6.  The golden comparisons reuse
the constants of tests/test_gpu_vae_train.py and tests/test_gpu_parity.py, attention the 2e-6 of
tests/test_gpu_attention.py.
Chamfer 1e-4 relative to the float64 oracle fed the device's own samples (fp32 differences and sums of 2048 terms)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import common as C
import recon_oracle as RO
from test_gpu_parity import close, dev, load, tiny
from test_gpu_vae_train import load_vae, sub_close, train_case

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

IDS = [7, 3, 1000000007]           # explicit, non-contiguous, unordered shape ids


def _meshes():
    tri = (np.array([[0.2, 0.1, 0.0], [1.3, 0.4, 0.2], [0.5, 1.1, 0.9]], np.float32), np.array([[0, 1, 2]], np.int32))
    tet = RO.tetrahedron()
    v, f = RO.cube_mesh(0.4, (0.3, -0.2, 0.1))
    zero = (v, np.concatenate([[[2, 2, 5]], f[:6], [[1, 7, 7]], f[6:], [[0, 0, 0]]]).astype(np.int32))
    return tri, tet, zero, RO.height_field()


def _check_oriented(meshes, n, normalize, ids, seed=11):
    from octfusion_amd import metrics
    pts, nrm = metrics.sample_surface(meshes, n=n, seed=seed, normalize=normalize, ids=ids, normals=True)
    plain = metrics.sample_surface(meshes, n=n, seed=seed, normalize=normalize, ids=ids)
    assert pts.shape == nrm.shape == (len(meshes), n, 3)
    assert torch.equal(pts, plain)                                               # the same bits as the unoriented call
    pts2, nrm2 = metrics.sample_surface(meshes, n=n, seed=seed, normalize=normalize, ids=ids, normals=True)
    assert torch.equal(pts, pts2) and torch.equal(nrm, nrm2)                     # two calls, identical bits
    got = nrm.double().cpu().numpy()
    assert np.abs(np.linalg.norm(got, axis=2) - 1.0).max() <= 1e-6
    for b, (v, f) in enumerate(meshes):
        sid = b if ids is None else ids[b]
        p_o, n_o, t = RO.sample_surface_oriented(v, f, n, seed=seed, shape=sid, normalize=normalize)
        assert RO.face_normals(v, f)[1][t].min() > 0.0                           # the oracle never draws a flat face
        err = np.abs(got[b] - n_o).max()
        assert err <= 1e-5, (b, err)
        assert np.abs(pts[b].double().cpu().numpy() - p_o).max() <= 1e-5 * max(1.0, np.abs(p_o).max())


@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('n', [1, 65, 2048])
def test_oriented_sampler_vs_oracle(n, normalize):
    """One triangle; a tetrahedron; a cube with three exactly zero-area faces (first, middle, last) among real ones -- a
    sample on one of them would carry a zero normal and miss both the unit-length and the oracle check; and a batch of
    1 / 4 / 300 faces in one call with explicit ids.  n: one point, one past a wavefront, the metrics size."""
    tri, tet, zero, sheet = _meshes()
    for m in (tri, tet, sheet):
        assert RO.min_angles_deg(*m).min() >= 10.0
    _check_oriented([tri], n, normalize, None)
    _check_oriented([tet], n, normalize, None)
    _check_oriented([zero], n, normalize, [5])
    _check_oriented([tri, tet, sheet], n, normalize, IDS)


def test_oriented_sampler_sliver_and_arguments():
    """A 0.1 degree sliver in a tilted plane: unit length and the oracle's direction (no 1e-5 claim there)."""
    from octfusion_amd import _lib, metrics
    a = math.radians(0.1)
    R = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])        # a rotation
    v = (np.array([[0, 0, 0], [1, 0, 0], [math.cos(a), math.sin(a), 0]]) @ R.T + [3.0, -2.0, 5.0]).astype(np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    assert RO.min_angles_deg(v, f).min() < 0.11
    pts, nrm = metrics.sample_surface([(v, f)], n=65, seed=2, normalize=True, normals=True)
    got = nrm[0].double().cpu().numpy()
    assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() <= 1e-6
    assert (got @ RO.face_normals(v, f)[0][0]).min() > 0.999
    # the entry point refuses a missing normals buffer instead of writing through NULL
    x = torch.zeros(16, device=dev())
    rc = _lib.lib().ofx_surface_sample_oriented(x.data_ptr(), x.data_ptr(), x.data_ptr(), None, 1, 1, 1, 0, 0,
                                                x.data_ptr(), x.data_ptr(), None, None)
    assert rc != 0


# ------------------------------------------------------------------------------------------------ entry points
def _points_octree(depth=6, fd=2):
    from octfusion_amd.octree import Points, build_octree_batch
    cl = [C.surface_points(3000, 41, 'sphere'), C.surface_points(2500, 42, 'torus')]
    pts = [Points(p.to(dev()), n.to(dev())) for p, n in cl]
    for p in pts:
        p.clip(-1.0, 1.0)
    return build_octree_batch(pts, depth, fd)


def _tiny_vae(golden):
    from octfusion_amd.graph_vae import GraphVAE
    G = golden('g_vae_enc')
    return load(GraphVAE(**G['cfg']), G['keys']), G


def test_extract_code_golden_and_composition(golden):
    from octfusion_amd.dual_octree import DualOctree
    from octfusion_amd.octree import split2octree_large
    vae, G = _tiny_vae(golden)
    oc, _ = tiny(G['split_small'])
    oc_l = split2octree_large(oc, G['split_large'].to(dev()), 4)
    n6 = DualOctree(oc_l).csr(6)[2]
    data = C.rand_input('vae_enc_in', n6, 4).to(dev())
    n4 = G['kl'].shape[0]
    code, doc = vae.extract_code(oc_l, noise=torch.zeros(n4, 3, device=dev()), data=data)
    assert isinstance(doc, DualOctree) and doc.octree is oc_l
    close(code, G['kl'][:, :3], 1e-3)                                            # zero noise: the code is the mean
    _, mean, logvar = vae.encode(data, doc, sample=False)                       # on the doctree extract_code returned
    close(torch.cat([mean, logvar], 1), G['kl'].clamp(min=-1e30), 1e-3)
    close(vae.octree_encoder_step(data, doc)[4][::8], G['h_rows8'], 1e-3)
    noise = C.rand_input('recon_noise', n4, 3).to(dev())
    code1, _ = vae.extract_code(oc_l, noise=noise, data=data)
    torch.testing.assert_close(code1, mean + torch.exp(0.5 * logvar) * noise)
    # an octree built from points brings its own feature
    ocp = _points_octree()
    docp = DualOctree(ocp)
    noise = C.rand_input('recon_noise_p', docp.csr(4)[2], 3).to(dev())
    want = vae.encode(docp.get_input_feature(), docp, noise=noise)[0]
    got, _ = vae.extract_code(ocp, noise=noise)
    assert torch.equal(got, want)


def test_forward_against_the_reference_training_forward(golden):
    """GraphVAE.forward(octree_in, octree_gt, pos) as the reference ran it for g_vae_train.pt."""
    G = golden('g_vae_train')
    vae = load_vae(G)
    oc_l, doc_l, data, noise = train_case(G)
    pos = G['pos'].to(dev())
    out = vae.forward(oc_l, oc_l, pos, noise=noise, data=data)
    assert set(out) == {'logits', 'reg_voxs', 'octree_out', 'kl_loss', 'code_max', 'code_min', 'neural_mpu', 'mpus'}
    assert set(vae.forward(oc_l, oc_l, noise=noise, data=data)) == set(out) - {'mpus'}
    assert out['octree_out'] is oc_l
    for d in (4, 5, 6):
        sub_close(out['logits'][d], G['logits'][d], 1e-3)
        sub_close(out['reg_voxs'][d], G['reg_voxs'][d], 1e-3)
        close(out['mpus'][d][0], G['sdf'][d], 1e-3)
    v = G['losses']['kl_loss']
    got = float(out['kl_loss']) * G['kl_weight']
    assert abs(got - v) <= 5e-4 * abs(v) + 1e-6, (got, v)
    code, _ = vae.extract_code(oc_l, noise=noise, data=data)
    assert float(out['code_max']) == float(code.max()) and float(out['code_min']) == float(code.min())
    # neural_mpu: depth_stop by default (the reference's forward wrapper), any decoded depth on request
    assert torch.equal(out['neural_mpu'](pos), out['mpus'][4][0])
    out6 = vae.forward(oc_l, oc_l, pos, noise=noise, data=data, mpu_depth=6)
    assert torch.equal(out6['neural_mpu'](pos), out6['mpus'][6][0])
    with pytest.raises(ValueError):
        vae.forward(oc_l, oc_l, noise=noise, data=data, mpu_depth=7)


def test_forward_evaluate_is_extract_plus_decode(golden):
    from octfusion_amd.dual_octree import DualOctree
    vae, _ = _tiny_vae(golden)
    oc = _points_octree()
    n4 = DualOctree(oc).csr(4)[2]
    noise = C.rand_input('recon_noise_e', n4, 3).to(dev())
    out = vae.forward(oc, evaluate=True, noise=noise)
    code, doc = vae.extract_code(oc, noise=noise)
    ref = vae.decode_code(code, doc, update_octree=True)
    assert set(out['logits']) == set(ref['logits']) == {4, 5, 6}
    for d in (4, 5, 6):
        assert torch.equal(out['logits'][d], ref['logits'][d]) and torch.equal(out['reg_voxs'][d], ref['reg_voxs'][d])
    a, b = out['octree_out'], ref['octree_out']
    assert a is not oc and a.depth == b.depth == 6
    assert torch.equal(a.nnum, b.nnum) and torch.equal(a.nnum_nempty, b.nnum_nempty)
    for d in range(7):
        assert torch.equal(a.keys[d], b.keys[d]) and torch.equal(a.children[d], b.children[d])
    # the draw count on torch's generator: two under evaluate (the second is the code), one otherwise
    _, mean, logvar = vae.encode(doc.get_input_feature(), doc, sample=False)
    for evaluate, draws in ((True, 2), (False, 1)):
        torch.manual_seed(123)
        o = vae.forward(oc, evaluate=evaluate)
        state = torch.cuda.get_rng_state(dev())
        torch.manual_seed(123)
        for _ in range(draws):
            eps = torch.randn_like(mean)
        assert torch.equal(torch.cuda.get_rng_state(dev()), state)
        z = mean + torch.exp(0.5 * logvar) * eps
        assert float(o['code_max']) == float(z.max()) and float(o['code_min']) == float(z.min())
    # given noise draws nothing
    torch.manual_seed(5)
    s0 = torch.cuda.get_rng_state(dev())
    vae.forward(oc, evaluate=True, noise=noise)
    assert torch.equal(torch.cuda.get_rng_state(dev()), s0)


@pytest.mark.parametrize('T', [5, 65])
def test_qkv_attention_forward(T):
    """modules.py:538-547 in float64 on the reference's tensor: [N * heads, 3 * ch, T], channels q | k | v."""
    from octfusion_amd.graph_unet_lr import QKVAttention
    N, heads, ch = 2, 2, 8
    qkv = C.rand_input('qkv_attention_%d' % T, N * heads, 3 * ch, T) * 1.5
    q, k, v = torch.split(qkv.double(), ch, dim=1)
    scale = 1 / math.sqrt(math.sqrt(ch))
    w = torch.softmax(torch.einsum('bct,bcs->bts', q * scale, k * scale), dim=-1)
    ref = torch.einsum('bts,bcs->bct', w, v)
    y = QKVAttention()(qkv.to(dev()))
    assert y.shape == (N * heads, ch, T) and y.dtype == torch.float32
    e = float((y.double().cpu() - ref).abs().max() / ref.abs().max())
    assert e < 2e-6, e


# ------------------------------------------------------------------------------------------------ driver
def _box_points(n, half, seed):
    """Oriented points on the surface of the cube [-half, half]^3."""
    rng = np.random.default_rng(seed)
    face = rng.integers(0, 6, n)
    uv = rng.uniform(-half, half, (n, 2))
    p, nn = np.zeros((n, 3)), np.zeros((n, 3))
    ax, sg = face // 2, (face % 2) * 2.0 - 1.0
    for i in range(3):
        m = ax == i
        p[m, i] = sg[m] * half
        nn[m, i] = sg[m]
        p[m, (i + 1) % 3] = uv[m, 0]
        p[m, (i + 2) % 3] = uv[m, 1]
    return p.astype(np.float32), nn.astype(np.float32)


def _check_outputs(out_dir, res, expect):
    from octfusion_amd import mesh
    saved = json.load(open(os.path.join(out_dir, 'metrics.json')))
    assert set(saved['shapes']) == set(res['shapes']) == set(expect)
    for name, (kind, pts, nrm) in expect.items():
        rec = saved['shapes'][name]
        assert rec['gt'] == kind and rec['input_points'] == len(pts)
        p, q = mesh.read_ply(os.path.join(out_dir, name, 'input.ply'))
        assert np.array_equal(p, pts) and np.array_equal(q, nrm)
        obj = os.path.join(out_dir, name, '0.obj')
        if rec['faces']:
            assert rec['obj'] == os.path.join(name, '0.obj')
            v, f = mesh.read_obj(obj)
            assert len(v) == rec['vertices'] and len(f) == rec['faces'] and f.min() >= 0 and f.max() < len(v)
            assert rec['chamfer_a'] > 0 and rec['chamfer_b'] > 0 and math.isfinite(rec['chamfer_a'] + rec['chamfer_b'])
        else:                                      # random weights may give no surface: the null path, no file
            assert rec['obj'] is None and not os.path.exists(obj)
            assert rec['chamfer_a'] is None and rec['chamfer_b'] is None


def test_driver_end_to_end(golden, tmp_path):
    from octfusion_amd import configs, mesh, metrics, reconstruct as R, synthetic
    from octfusion_amd.graph_vae import GraphVAE
    kw = {k: v for k, v in golden('g_vae_enc')['cfg'].items()}
    ps = 0.5
    # ---- two pointcloud.npz shapes (file units: [-1, 1] * point_scale), through the function, two calls of one shape
    sp, sn = C.surface_points(4000, 9, 'sphere')
    bp, bn = _box_points(4000, 0.6, 3)
    expect = {}
    for name, p, n in (('ball', sp.numpy(), sn.numpy()), ('box.v1', bp, bn)):
        d = tmp_path / 'data' / name
        d.mkdir(parents=True)
        np.savez(str(d / 'pointcloud.npz'), points=p * ps, normals=n)
        q = (p * np.float32(ps)) / np.float32(ps)
        keep = ((q > -1) & (q < 1)).all(1)
        expect[name[:name.rfind('.')] if '.' in name else name] = ('points', q[keep], n[keep])
    vae = GraphVAE(**kw)
    vae.load_state_dict(synthetic.random_state_dict(vae))
    vae = vae.to(dev()).eval()
    cfg = {'depth': kw['depth'], 'full_depth': kw['full_depth'], 'point_scale': ps}
    inputs = R.read_inputs([str(tmp_path / 'data' / 'ball'), str(tmp_path / 'data' / 'box.v1')])
    out_dir = str(tmp_path / 'recon')
    res = R.reconstruct(vae, cfg, inputs, dev(), sdf_resolution=32, batch=1, seed=4, chamfer_points=2048,
                        out_dir=out_dir)
    assert res['mpu_depth'] == kw['depth_out']
    _check_outputs(out_dir, res, expect)
    # ---- the same box as an OBJ, through the command line
    configs.CONFIGS['tiny_recon'] = configs.CONFIGS['snet_uncond']
    configs.VAES['tiny_recon'] = kw
    mesh.MESH_SCALES['tiny_recon'] = ps
    try:
        v, f = RO.cube_mesh(0.3)
        mesh.write_obj(str(tmp_path / 'cube.obj'), v, f)
        out2 = str(tmp_path / 'recon_mesh')
        res2 = R.main(['--config', 'tiny_recon', '--from-mesh', '--input', str(tmp_path / 'cube.obj'), '--out', out2,
                       '--sdf-resolution', '32', '--points', '4000', '--chamfer-points', '2048', '--seed', '4'])
    finally:
        del configs.CONFIGS['tiny_recon'], configs.VAES['tiny_recon'], mesh.MESH_SCALES['tiny_recon']
    v2, f2 = mesh.read_obj(str(tmp_path / 'cube.obj'))
    p, n = metrics.sample_surface([(v2, f2)], n=4000, seed=4, normalize=True, ids=[0], normals=True)
    p = p[0] * 0.9                                   # --fit defaults to sdf_scale
    keep = ((p > -1) & (p < 1)).all(1)
    assert bool(keep.all())
    _check_outputs(out2, res2, {'cube': ('mesh', p.cpu().numpy(), n[0].cpu().numpy())})
    assert res2['fit'] == 0.9 and res2['config'] == 'tiny_recon'


def test_chamfer_score():
    from octfusion_amd import metrics, reconstruct as R
    a = tuple(torch.from_numpy(x).to(dev()) for x in RO.cube_mesh(0.5))
    b = tuple(torch.from_numpy(x).to(dev()) for x in RO.cube_mesh(0.5, (0.25, 0.1, 0.0)))
    assert R.chamfer(a, a, 2048, seed=6) == (0.0, 0.0)
    ca, cb = R.chamfer(a, b, 2048, seed=6)
    pa = metrics.sample_surface([a], n=2048, seed=6, normalize=False)[0].double().cpu().numpy()
    pb = metrics.sample_surface([b], n=2048, seed=6, normalize=False)[0].double().cpu().numpy()
    wa, wb = RO.chamfer(pa, pb)
    assert abs(ca - wa) <= 1e-4 * wa and abs(cb - wb) <= 1e-4 * wb, (ca, wa, cb, wb)
    assert ca != cb                                   # directed terms, in the reference's order
    # a given cloud on the gt side (the point-cloud input of the driver) is taken as it is
    cloud = torch.from_numpy(pa[:1000]).float().to(dev())
    ga, gb = R.chamfer(cloud, b, 2048, seed=6)
    wa, wb = RO.chamfer(pa[:1000].astype(np.float32), pb)
    assert abs(ga - wa) <= 1e-4 * wa and abs(gb - wb) <= 1e-4 * wb
