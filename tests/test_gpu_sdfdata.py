"""GPU tests of the training-data samplers (csrc/ofx_sdfdata.hip, octfusion_amd/dataset.py) against the numpy oracle
(tests/sdfdata_oracle.py) on a sphere SDF: centre (0.07, -0.05, 0.03), radius 0.55, lattice index i at i/(S/2) - 1.

Tolerances.  points: bit-equal (the position arithmetic is exact fp32 on both sides).  sdf: one fp16 ulp -- both sides
round a value whose fp32-vs-fp64 difference is far below half an ulp, so they can land on adjacent fp16 numbers.
grad: 2^-10 + 1e-4 absolute -- one fp16 ulp in [0.5, 1] is 2^-10; twelve fp32 operations on values <= 2 give at most
~1e-6, and dividing by a gradient-sum norm >= 0.1 (asserted on the oracle's samples; the smallest seen is 0.13) stays
below 1e-4.  Occupancy bits: equal wherever the oracle's |value| >= 1e-5 (at most 0.1 % may be left out; this sphere
leaves out none)."""
import numpy as np
import pytest
import torch

import sdfdata_oracle as O

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

K = 4


def dev():
    return torch.device('cuda:0')


def bits16(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else t
    assert a.dtype == np.float16
    return a.view(np.uint16)


def ordered16(t):
    """fp16 values as integers in which adjacent numbers differ by one."""
    b = bits16(t).astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7fff), b)


def check_samples(got, ref):
    n = int(ref['keep'].sum())
    print('kept %d of %d candidates (oracle %d)' % (got['sdf'].shape[0], len(ref['keep']), n))
    assert got['points'].shape == (n, 3) and got['grad'].shape == (n, 3) and got['sdf'].shape == (n,)
    assert got['points'].dtype == got['grad'].dtype == got['sdf'].dtype == torch.float16
    assert np.array_equal(bits16(got['points']), bits16(ref['points']))
    ulp = np.abs(ordered16(got['sdf']) - ordered16(ref['sdf'])).max() if n else 0
    gerr = np.abs(got['grad'].cpu().numpy().astype(np.float64) - ref['grad'].astype(np.float64)).max() if n else 0.0
    print('sdf: max %d fp16 ulp; grad: max abs error %.3e' % (ulp, gerr))
    assert ulp <= 1
    assert gerr <= 2.0 ** -10 + 1e-4


def same_bits(a, b):
    return all(torch.equal(a[k].view(torch.int16), b[k].view(torch.int16)) for k in ('points', 'grad', 'sdf'))


def hash_u(seed, shape, n, shift, scale, dtype):
    from octfusion_amd import _lib
    h = _lib.lib().ofx_metrics_hash
    return np.array([[(h(seed, shape, g, c) >> shift) * scale for c in range(3)] for g in range(n)], dtype)


@pytest.fixture(scope='module')
def case16():
    """S = 16, every node of depths 2 and 3, four samples each: 2304 candidates, the oracle's answer computed once."""
    sdf = O.sphere_lattice(16)
    xyz, off = O.full_nodes((2, 3))
    u = np.random.RandomState(16).rand(len(xyz) * K, 3).astype(np.float32)
    return {'sdf': sdf, 'xyz': xyz, 'off': off, 'u': u, 'ref': O.sample_sdf(sdf, xyz, off, 2, K, u)}


def test_sample_nodes_vs_oracle(case16):
    from octfusion_amd import dataset as D
    c = case16
    assert len(c['xyz']) * K == 2304
    dropped = 1.0 - c['ref']['keep'].mean()
    assert 0.1 < dropped < 0.25                      # roughly a sixth lies beyond S - 1
    assert c['ref']['grad_sum_norm'].min() >= 0.1
    got = D.sample_nodes(c['sdf'], c['xyz'], c['off'], 2, K, u=c['u'])
    check_samples(got, c['ref'])


def test_sample_nodes_boundary():
    """Hand-placed uniforms at depth 3 of S = 16 (scale 2, limit 15).  The lattice is the head of a longer buffer whose
    tail is NaN: a read past corner index S - 1 would turn the value into NaN."""
    from octfusion_amd import dataset as D
    S = 16
    buf = torch.full((S ** 3 + 4 * S * S,), float('nan'), dtype=torch.float32, device=dev())
    lat = O.sphere_lattice(S)
    buf[:S ** 3] = torch.from_numpy(lat).reshape(-1).to(dev())
    sdf = buf[:S ** 3].view(S, S, S)
    below = np.float32(0.5) - np.float32(2.0 ** -21)          # (7 + below) * 2 = the largest fp32 below 15
    assert (np.float32(7) + below) * np.float32(2) == np.nextafter(np.float32(15), np.float32(0))
    last = np.float32(1) - np.float32(2.0 ** -24)
    assert np.float32(7) + last == np.float32(8) and np.float32(3) + last == np.float32(4)
    xyz = np.array([[7, 7, 7]] * 2 + [[3, 3, 3], [7, 0, 0]], np.int32)
    u = np.zeros((4, 1, 3), np.float32)
    u[0, 0] = [0.5, 0.25, 0.25]          # x lands exactly on S - 1: dropped
    u[1, 0] = below                      # all three axes just below S - 1: kept, upper corners have index S - 1
    u[2, 0] = last                       # 3 + u rounds to 4: kept, in the next cell
    u[3, 0] = [last, 0.5, 0.5]           # 7 + u rounds to 8 -> 16 >= 15: dropped
    ref = O.sample_sdf(lat, xyz, [0, 4], 3, 1, u)
    assert ref['keep'].tolist() == [False, True, True, False]
    assert ref['pos'][0].tolist() == [float(np.nextafter(np.float32(15), np.float32(0)))] * 3
    assert ref['pos'][1].tolist() == [8.0, 8.0, 8.0]
    got = D.sample_nodes(sdf, xyz, [0, 4], 3, 1, u=u)
    assert torch.isfinite(got['sdf'].float()).all() and torch.isfinite(got['grad'].float()).all()
    check_samples(got, ref)


def test_sample_nodes_hash_mode(case16):
    """u=None draws (ofx_metrics_hash(seed, shape, i*k + j, axis) >> 40) * 2^-24: bit-equal to passing those uniforms,
    reproducible, and keyed by the shape id."""
    from octfusion_amd import dataset as D
    c = case16
    seed, shape = 1234, 77
    u = hash_u(seed, shape, len(c['xyz']) * K, 40, 2.0 ** -24, np.float32)
    assert 0.0 <= u.min() and u.max() < 1.0
    a = D.sample_nodes(c['sdf'], c['xyz'], c['off'], 2, K, seed=seed, shape_id=shape)
    b = D.sample_nodes(c['sdf'], c['xyz'], c['off'], 2, K, u=u)
    assert a['sdf'].shape[0] > 1500 and a['sdf'].shape == b['sdf'].shape and same_bits(a, b)
    again = D.sample_nodes(c['sdf'], c['xyz'], c['off'], 2, K, seed=seed, shape_id=shape)
    assert same_bits(a, again)
    other = D.sample_nodes(c['sdf'], c['xyz'], c['off'], 2, K, seed=seed, shape_id=shape + 1)
    assert other['sdf'].shape != a['sdf'].shape or not same_bits(a, other)
    check_samples(a, O.sample_sdf(c['sdf'], c['xyz'], c['off'], 2, K, u))


def sphere_cloud(n, seed, radius=0.55, centre=(0.07, -0.05, 0.03)):
    g = torch.Generator().manual_seed(seed)
    nrm = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    return nrm * radius + torch.tensor(centre), nrm


def test_sample_sdf_on_a_built_octree():
    """Irregular node lists: the octree of ~2000 sphere surface points at depth 4 / full_depth 2, S = 32.  Count and
    order against the oracle fed with the same node coordinates; an empty node list gives count 0."""
    from octfusion_amd import dataset as D
    from octfusion_amd.octree import Octree, Points
    pts, nrm = sphere_cloud(2000, 4)
    oc = Octree(4, 2, 1, dev()).build_octree(Points(pts.to(dev()), nrm.to(dev())))
    counts = [int(oc.nnum[d]) for d in (2, 3, 4)]
    print('nodes per depth', counts)
    assert counts[0] == 64 and any(c % 64 for c in counts[1:])
    xyz = np.concatenate([torch.stack(oc.xyzb(d)[:3], 1).cpu().numpy() for d in (2, 3, 4)]).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(counts)]).tolist()
    sdf = O.sphere_lattice(32)
    u = np.random.RandomState(32).rand(len(xyz) * K, 3).astype(np.float32)
    ref = O.sample_sdf(sdf, xyz, off, 2, K, u)
    assert ref['grad_sum_norm'].min() >= 0.1
    check_samples(D.sample_sdf(sdf, oc, 2, 4, K, u=u), ref)
    empty = D.sample_nodes(sdf, np.zeros((0, 3), np.int32), [0, 0], 2, K)
    assert empty['points'].shape == (0, 3) and empty['grad'].shape == (0, 3) and empty['sdf'].shape == (0,)


@pytest.mark.parametrize('n', [4099, 5])
def test_sample_occu_vs_oracle(n):
    from octfusion_amd import dataset as D
    sdf = O.sphere_lattice(32)
    u = np.random.RandomState(n).rand(n, 3)
    ref = O.sample_occu(sdf, u)
    got = D.sample_occu(sdf, n, u=u)
    assert got['occupancies'].dtype == torch.uint8 and got['occupancies'].shape == ((n + 7) // 8,)
    assert np.array_equal(bits16(got['points']), bits16(ref['points']))
    near = np.abs(ref['value']) < 1e-5
    print('%d of %d points within 1e-5 of the surface; %d inside' % (near.sum(), n, (ref['value'] < 0).sum()))
    assert near.mean() <= 1e-3
    have = got['occupancies'].cpu().numpy()
    if not near.any():
        assert np.array_equal(have, ref['occupancies'])
    assert np.array_equal(np.unpackbits(have)[:n][~near], (ref['value'] < 0)[~near])
    assert not np.unpackbits(have)[n:].any()         # zero padding
    # hash mode: 53 bits of the same counter hash, bit-equal to passing them
    uh = hash_u(9, 5, n, 11, 2.0 ** -53, np.float64)
    a, b = D.sample_occu(sdf, n, seed=9, shape_id=5), D.sample_occu(sdf, n, u=uh)
    assert torch.equal(a['occupancies'], b['occupancies'])
    assert torch.equal(a['points'].view(torch.int16), b['points'].view(torch.int16))


def test_dataset_folder_to_training_step(tmp_path):
    """The driver writes a two-shape dataset folder from lattices + point clouds; ReadFile -> TransformShape -> collate
    -> to_device_batch -> one vae_stage_step on it."""
    from octfusion_amd import dataset as D
    from octfusion_amd import synthetic, training as T, vae_training as VT
    from octfusion_amd.graph_vae import GraphVAE
    from octfusion_amd.mesh import read_ply
    S, names, radii = 32, ['cat/a', 'cat/b'], [0.55, 0.4]
    sdf_dir, data_dir = tmp_path / 'sdf', tmp_path / 'dataset'
    for name, r in zip(names, radii):
        (sdf_dir / 'cat').mkdir(parents=True, exist_ok=True)
        (data_dir / name).mkdir(parents=True)
        np.save(str(sdf_dir / (name + '.npy')), O.sphere_lattice(S, radius=r))
        pts, nrm = sphere_cloud(3000, 1, radius=r)
        np.savez(str(data_dir / name / 'pointcloud.npz'), points=(pts * 0.5).numpy().astype(np.float16),
                 normals=nrm.numpy().astype(np.float16))
    argv = ['--sdf-dir', str(sdf_dir), '--dataset-dir', str(data_dir), '--depth', '4', '--full-depth', '2', '--occu',
            '--test-points']
    D.main(argv)
    for name in names:
        with np.load(str(data_dir / name / 'sdf.npz')) as z:
            n = z['sdf'].shape[0]
            assert n > 1000 and z['points'].shape == (n, 3) and z['grad'].shape == (n, 3)
            assert z['points'].dtype == z['grad'].dtype == z['sdf'].dtype == np.float16
            assert np.abs(z['points'].astype(np.float32)).max() <= 0.5
            # the samples carry the sphere's distance field: |p| - r, in [-1, 1] units
            p = z['points'].astype(np.float64) / 0.5
            d = np.linalg.norm(p - np.array([0.07, -0.05, 0.03]), axis=1) - radii[names.index(name)]
            # a trilinear interpolant of a 1-Lipschitz field is off by at most the cell diagonal; fp16 adds 2^-11
            assert np.abs(z['sdf'].astype(np.float64) - d).max() < np.sqrt(3) * 2 / S + 2.0 ** -10
        with np.load(str(data_dir / name / 'points.npz')) as z:
            assert z['points'].shape == (100000, 3) and z['occupancies'].shape == (12500,)
        ply, _ = read_ply(str(tmp_path / 'test.input' / (name + '.ply')))
        assert ply.shape == (3000, 3)
    stamp = {n: (data_dir / n / 'sdf.npz').stat().st_mtime_ns for n in names}
    D.main(argv)                                     # existing outputs are skipped
    assert stamp == {n: (data_dir / n / 'sdf.npz').stat().st_mtime_ns for n in names}

    flags = {'depth': 4, 'full_depth': 2, 'point_scale': 0.5, 'point_sample_num': 300, 'load_pointcloud': True,
             'load_sdf': True, 'load_occu': False, 'sample_surf_points': False}
    read, transform = D.ReadFile(flags), D.TransformShape(flags, seed=3)
    batch = D.collate([transform(read(str(data_dir / n)), i) for i, n in enumerate(names)])
    again = D.collate([transform(read(str(data_dir / n)), i) for i, n in enumerate(names)])
    assert torch.equal(batch['pos'], again['pos'])   # seeded
    args = D.to_device_batch(batch, flags)
    pos = args['pos']
    assert pos.shape == (600, 4) and pos.is_cuda and pos.dtype == torch.float32
    assert pos[:, 3].tolist() == [0.0] * 300 + [1.0] * 300
    assert float(pos[:, :3].abs().max()) <= 1.0
    assert args['sdf_gt'].shape == (600,) and args['grad_gt'].shape == (600, 3)
    assert args['doctree_in'].octree.batch_size == 2
    vae = GraphVAE(depth=4, channel_in=4, nout=4, full_depth=2, depth_stop=3, depth_out=4, resblk_type='basic',
                   resblk_num=2, code_channel=16, embed_dim=3)
    vae.load_state_dict(synthetic.random_state_dict(vae))
    vae = vae.to(dev())
    opt = T.AdamW(vae.named_parameters(), lr=1e-5)
    losses = VT.vae_stage_step(vae, opt, **args)
    assert {'loss', 'kl_loss', 'sdf_loss_3', 'sdf_loss_4', 'grad_loss_4', 'loss_4'} <= set(losses)
    assert all(bool(torch.isfinite(v).all()) for v in losses.values())

    surf = D.TransformShape(dict(flags, sample_surf_points=True, load_sdf=False), seed=3)
    out = surf(D.ReadFile(dict(flags, load_sdf=True))(str(data_dir / names[0])), 0)
    assert out['pos'].shape == (600, 3) and out['sdf'][:300].eq(0).all() and out['sdf'][300:].eq(-1).all()
