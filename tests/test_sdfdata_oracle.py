"""CPU checks of the training-data path (octfusion_amd/dataset.py) and of its numpy oracle (tests/sdfdata_oracle.py):
the bit packing, the files' layout and the collate's batch column.  No GPU."""
import numpy as np
import pytest
import torch

import sdfdata_oracle as O


@pytest.mark.parametrize('n', [5, 8, 4099])
def test_oracle_packing_is_numpy_packbits(n):
    bits = np.random.RandomState(n).rand(n) < 0.5
    got = O.packbits(bits)
    assert got.dtype == np.uint8 and got.shape == ((n + 7) // 8,)
    assert np.array_equal(got, np.packbits(bits))


def test_oracle_test_field_needs_no_exclusions():
    """The sphere of the GPU tests: no sample has a near-zero gradient sum (the normalisation is well conditioned) and
    no occupancy point sits within 1e-5 of the surface (every bit is decided)."""
    for S, depths in ((16, (2, 3)), (32, (2, 3, 4))):
        sdf = O.sphere_lattice(S)
        xyz, off = O.full_nodes(depths)
        u = np.random.RandomState(S).rand(len(xyz) * 4, 3).astype(np.float32)
        ref = O.sample_sdf(sdf, xyz, off, depths[0], 4, u)
        assert ref['grad_sum_norm'].min() > 0.1
        assert 0 < ref['keep'].sum() < len(ref['keep'])
    occ = O.sample_occu(O.sphere_lattice(32), np.random.RandomState(3).rand(4099, 3))
    assert np.abs(occ['value']).min() > 1e-5


def test_written_files_have_the_reference_layout(tmp_path):
    """sdf.npz: points [n, 3], grad [n, 3], sdf [n] fp16; points.npz: points [n, 3] fp16, occupancies [ceil(n/8)] uint8
    (tools/repair_mesh.py:338, 378) -- and ReadFile hands them back under the reference's keys."""
    from octfusion_amd import dataset as D
    sdf = O.sphere_lattice(16)
    xyz, off = O.full_nodes((2, 3))
    ref = O.sample_sdf(sdf, xyz, off, 2, 4, np.random.RandomState(0).rand(len(xyz) * 4, 3))
    occ = O.sample_occu(sdf, np.random.RandomState(1).rand(4099, 3))
    shape = tmp_path / 'a'
    shape.mkdir()
    D.write_sdf_npz(str(shape / 'sdf.npz'), {k: torch.from_numpy(ref[k]) for k in ('points', 'grad', 'sdf')})
    D.write_occu_npz(str(shape / 'points.npz'), occ)
    n = int(ref['keep'].sum())
    with np.load(str(shape / 'sdf.npz')) as z:
        assert sorted(z.files) == ['grad', 'points', 'sdf']
        assert z['points'].dtype == z['grad'].dtype == z['sdf'].dtype == np.float16
        assert z['points'].shape == (n, 3) and z['grad'].shape == (n, 3) and z['sdf'].shape == (n,)
        assert np.array_equal(z['sdf'].view(np.uint16), ref['sdf'].view(np.uint16))
    with np.load(str(shape / 'points.npz')) as z:
        assert sorted(z.files) == ['occupancies', 'points']
        assert z['points'].dtype == np.float16 and z['points'].shape == (4099, 3)
        assert z['occupancies'].dtype == np.uint8 and z['occupancies'].shape == (513,)
        assert np.array_equal(np.unpackbits(z['occupancies'])[:4099].astype(bool), occ['value'] < 0)
    with pytest.raises(ValueError):
        D.write_sdf_npz(str(shape / 'bad.npz'), {k: ref[k].astype(np.float32) for k in ('points', 'grad', 'sdf')})
    out = D.ReadFile({'load_sdf': True, 'load_occu': True})(str(shape))
    assert sorted(out) == ['occu', 'sdf'] and sorted(out['sdf']) == ['grad', 'points', 'sdf']
    assert out['occu']['occupancies'].shape == (513,)
    with pytest.raises(ValueError):
        D.ReadFile({'load_octree': True})


def test_collate_batch_column():
    """pos [n, 4]: xyz of the shapes in order, last column the shape's position in the batch (datasets/utils.py:19-23),
    for two shapes with different sample counts; sdf / grad concatenated alike."""
    from octfusion_amd import dataset as D
    g = torch.Generator().manual_seed(0)
    a = {'pos': torch.rand(5, 3, generator=g), 'sdf': torch.rand(5, generator=g), 'grad': torch.rand(5, 3, generator=g),
         'points': 'cloud a'}
    b = {'pos': torch.rand(3, 3, generator=g), 'sdf': torch.rand(3, generator=g), 'grad': torch.rand(3, 3, generator=g),
         'points': 'cloud b'}
    out = D.collate([a, b])
    assert out['points'] == ['cloud a', 'cloud b']
    assert out['pos'].shape == (8, 4) and out['pos'].dtype == torch.float32
    assert out['pos'][:, 3].tolist() == [0.0] * 5 + [1.0] * 3
    assert torch.equal(out['pos'][:5, :3], a['pos']) and torch.equal(out['pos'][5:, :3], b['pos'])
    assert torch.equal(out['sdf'], torch.cat([a['sdf'], b['sdf']]))
    assert torch.equal(out['grad'], torch.cat([a['grad'], b['grad']]))
