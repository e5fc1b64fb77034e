"""CPU-side pins of the voxel-mesh oracle (tests/voxmesh_oracle.py) to the reference's own _voxel2mesh output
(tests/golden/g_voxmesh.pt, written by tests/golden/make_voxmesh_golden.py), of the oracle's welding rule, and of the
no-GPU / argument behaviour of octfusion_amd.voxmesh and the --octree-mesh flag."""
import numpy as np
import pytest
import torch

import voxmesh_oracle as O
from octfusion_amd import voxmesh

CASES = ['random2', 'random4', 'random8', 'checker8', 'sparse16', 'float4']


def test_golden_holds_the_case_list(golden):
    assert sorted(golden('g_voxmesh')) == sorted(CASES)


@pytest.mark.parametrize('name', CASES)
def test_oracle_reproduces_the_reference(golden, name):
    c = golden('g_voxmesh')[name]
    v, f = O.unwelded(c['grid'].numpy(), c['threshold'])
    assert c['verts'].dtype == torch.float32 and c['faces'].dtype == torch.int32
    assert v.dtype == np.float32 and f.dtype == np.int32
    assert np.array_equal(v, c['verts'].numpy())                 # order included
    assert np.array_equal(f, c['faces'].numpy())


@pytest.mark.parametrize('name', CASES)
def test_oracle_welding(golden, name):
    c = golden('g_voxmesh')[name]
    R = int(c['grid'].shape[0])
    v, f = c['verts'].numpy(), c['faces'].numpy()
    vw, fw = O.weld(v, f, R)
    assert np.array_equal(vw[fw], v[f])                          # the same triangles, corner by corner
    idx = O.corner_index(np.rint((vw.astype(np.float64) + 1) * (R / 2)).astype(np.int64), R)
    assert (np.diff(idx) > 0).all()                              # unique, in ascending corner order
    assert len(np.unique(vw, axis=0)) == len(vw)
    assert sorted(np.unique(fw).tolist()) == list(range(len(vw)))   # every welded vertex is used


def test_oracle_counts_and_winding():
    for R in (2, 4, 8):
        v, f = O.welded(np.ones((R, R, R), np.float32))
        assert len(f) == 2 * 6 * R * R and len(v) == (R + 1) ** 3 - (R - 1) ** 3
        assert O.directed_edge_balance(f) and O.signed_volume(v, f) == 8.0      # outward: positive volume
        v, f = O.unwelded(O.checkerboard(R))
        assert len(f) == 2 * 6 * R ** 3 // 2
    # a value equal to the threshold and non-finite values count as empty
    g = np.array([0.4, np.nan, np.inf, -np.inf, 0.5, 0.3, 1.0, 0.0], np.float32).reshape(2, 2, 2)
    assert O.occupancy(g, 0.4).ravel().tolist() == [False, False, False, False, True, False, True, False]


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_voxel_mesh_fails_loudly_without_gpu():
    from octfusion_amd import _lib
    with pytest.raises(_lib.OfxError):
        voxmesh.voxel_mesh(torch.zeros(1, 8, 8, 8))
    with pytest.raises(_lib.OfxError):
        voxmesh.octree_mesh(None, 5)


def test_generate_octree_mesh_without_out_raises():
    from octfusion_amd import generate as G
    with pytest.raises(ValueError, match='--octree-mesh needs --out'):
        G.main(['--config', 'snet_uncond', '--shapes', '1', '--no-vae', '--octree-mesh'])
