"""Voxel meshes on the device (csrc/ofx_voxmesh.hip through octfusion_amd.voxmesh) against the reference's own output
(tests/golden/g_voxmesh.pt) and the numpy oracle (tests/voxmesh_oracle.py).  Every comparison is exact: the
coordinates corner * 2 / R - 1 are exact in fp32."""
import os

import numpy as np
import pytest
import torch

import common as C
import voxmesh_oracle as O
from octfusion_amd.voxmesh import octree_mesh, voxel_mesh

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

CASES = ['random2', 'random4', 'random8', 'checker8', 'sparse16', 'float4']


def dev():
    return torch.device('cuda:0')


def host(m):
    assert m[0].dtype == torch.float32 and m[1].dtype == torch.int32
    assert m[0].dim() == 2 and m[0].shape[1] == 3 and m[1].dim() == 2 and m[1].shape[1] == 3
    return m[0].cpu().numpy(), m[1].cpu().numpy()


def to_dev(grids):
    return torch.from_numpy(np.stack(grids).astype(np.float32)).to(dev())


def check(grids, threshold=0.4):
    """Both variants of a batch against the oracle; returns the welded device meshes."""
    d = to_dev(grids)
    out = None
    for weld in (False, True):
        out = voxel_mesh(d, threshold, weld=weld)
        assert len(out) == len(grids)
        for g, m in zip(grids, out):
            v, f = host(m)
            wv, wf = O.mesh(g, threshold, weld)
            assert np.array_equal(f, wf) and np.array_equal(v, wv)
    return out


@pytest.mark.parametrize('name', CASES)
def test_golden_cases(golden, name):
    c = golden('g_voxmesh')[name]
    v, f = host(voxel_mesh(c['grid'].to(dev()), c['threshold'], weld=False)[0])
    assert np.array_equal(v, c['verts'].numpy()) and np.array_equal(f, c['faces'].numpy())


def corner_cells(R):
    g = np.zeros((R, R, R), np.float32)
    for x in (0, R - 1):
        for y in (0, R - 1):
            for z in (0, R - 1):
                g[x, y, z] = 1
    return g


# The mask words hold 64 cells.  R = 2: 8 bits, under one word; 4: the whole shape is one word; 8: rows inside a word,
# +-R^2 is a whole word; 16, 32: +-R shifts across two words; 64: a row is one word, so z never leaves it
# (test_z_crosses_a_word_mid_row has R = 128)
@pytest.mark.parametrize('R', [2, 4, 8, 16, 32, 64])
def test_mask_layout_edge_cases(R):
    full = np.ones((R, R, R), np.float32)
    empty = np.zeros((R, R, R), np.float32)
    out = check([empty, full, O.random_grid(R, 0.5, seed=R)])        # B = 3: offsets and per-shape index locality
    assert out[0][0].shape[0] == 0 and out[0][1].shape[0] == 0
    assert out[1][1].shape[0] == 2 * 6 * R * R                        # a full grid: 6 R^2 quads
    for v, f in out:
        if f.shape[0]:
            assert int(f.min()) == 0 and int(f.max()) == v.shape[0] - 1
    out = check([corner_cells(R), O.checkerboard(R)])
    assert out[0][1].shape[0] == (2 * 6 * 8 if R > 2 else 2 * 6 * 4)     # 8 lone cells; at R = 2 they are the full grid
    assert out[1][1].shape[0] == 2 * 6 * R ** 3 // 2                  # the capacity maximum


def test_z_crosses_a_word_mid_row():
    R = 128                                                           # a row is two words
    g = O.random_grid(R, 0.02, seed=1)
    g[5, 7, 60:70] = 1                                                # a rod through the word boundary
    g[64:66, 100, :] = 1                                              # whole rows
    g[20:30, 20:30, 63:65] = 1                                        # a slab on both sides of it
    g[R - 1, R - 1, R - 1] = 1
    check([g])


def test_single_grid_threshold_and_non_finite_values():
    g = O.random_grid(8, 0.5, seed=3) * 0.5 + 0.25                    # values 0.25 / 0.75
    g[1, 2, 3], g[4, 4, 4], g[0, 0, 0], g[7, 7, 7], g[3, 3, 3] = np.nan, np.inf, -np.inf, 0.5, 0.5
    check([g], threshold=0.5)                                         # == threshold and non-finite: empty
    m = voxel_mesh(torch.from_numpy(g).to(dev()), 0.5)                # [R, R, R] input
    wv, wf = O.welded(g, 0.5)
    assert len(m) == 1 and np.array_equal(host(m[0])[1], wf) and np.array_equal(host(m[0])[0], wv)


_OCTREES = {}


def octree(kind):
    from octfusion_amd import synthetic
    from octfusion_amd.octree import split2octree_small
    if kind not in _OCTREES:
        if kind == 'random5':
            _OCTREES[kind] = (split2octree_small(C.random_split_small(2, 3, 4).to(dev()), 5, 3), 5)
        else:
            _OCTREES[kind] = (split2octree_small(synthetic.shell6_split(2).to(dev()), 6, 4), 6)
    return _OCTREES[kind]


def scatter(oc, d):
    x, y, z, b = oc.xyzb(d)
    R = 1 << d
    grid = torch.zeros(oc.batch_size, R, R, R, device=dev())
    grid[b, x, y, z] = 1
    return grid


@pytest.mark.parametrize('kind', ['random5', 'shell6'])
@pytest.mark.parametrize('up', [0, 1])
def test_octree_front_end(kind, up):
    oc, depth = octree(kind)
    d = depth - up                                                    # the leaf depth and a non-leaf depth
    grid = scatter(oc, d)
    assert 0 < int(grid.sum()) == int(oc.nnum[d])
    for weld in (True, False):
        a, b = octree_mesh(oc, d, weld=weld), voxel_mesh(grid, weld=weld)
        assert len(a) == len(b) == oc.batch_size
        for (va, fa), (vb, fb) in zip(a, b):
            assert fa.shape[0] > 0 and torch.equal(va, vb) and torch.equal(fa, fb)
    if up == 0:                                                       # and against the oracle
        wv, wf = O.welded(grid[1].cpu().numpy())
        v, f = host(octree_mesh(oc, d)[1])
        assert np.array_equal(v, wv) and np.array_equal(f, wf)


def test_shell_mesh_is_closed_and_encloses_the_cells():
    oc, depth = octree('shell6')
    R = 1 << depth
    occupied = scatter(oc, depth).sum(dim=(1, 2, 3)).tolist()
    for n, m in zip(occupied, octree_mesh(oc, depth)):
        v, f = host(m)
        assert O.directed_edge_balance(f)
        want = n * (2.0 / R) ** 3                                     # exact in float64
        # the coordinates are exact and the sum is taken in float64: a few fp32 ulp of the total
        assert abs(O.signed_volume(v, f) - want) <= 4 * np.spacing(np.float32(want))


def test_interoperability(tmp_path):
    from octfusion_amd import mesh
    g = np.zeros((16, 16, 16), np.float32)
    g[1:5, 1:5, 1:5] = 1                                              # 4^3 cube
    g[10:12, 9:11, 12:14] = 1                                         # 2^3 cube, apart from it
    meshes = voxel_mesh(to_dev([g]))
    t = mesh.components(meshes)[0]
    assert t['n_faces'].tolist() == [2 * 6 * 16, 2 * 6 * 4] and t['n_verts'].tolist() == [98, 26]
    v, f = host(mesh.largest_component(meshes)[0])
    big = g.copy()
    big[10:12] = 0
    wv, wf = O.welded(big)
    assert np.array_equal(v, wv) and np.array_equal(f, wf)
    path = str(tmp_path / 'cubes.obj')
    assert mesh.write_obj(path, *meshes[0])
    rv, rf = mesh.read_obj(path)
    assert np.array_equal(rv, host(meshes[0])[0]) and np.array_equal(rf, host(meshes[0])[1])


def test_reproducible():
    d = to_dev([O.random_grid(32, 0.4, seed=s) for s in range(3)])
    for weld in (True, False):
        a, b = voxel_mesh(d, weld=weld), voxel_mesh(d, weld=weld)
        for (va, fa), (vb, fb) in zip(a, b):
            assert torch.equal(va, vb) and torch.equal(fa, fb)


def test_input_checks():
    ok = torch.zeros(1, 4, 4, 4, device=dev())
    for bad in (ok.double(), ok.cpu(), ok.int(), torch.zeros(1, 4, 4, 8, device=dev()),
                torch.zeros(1, 6, 6, 6, device=dev()), torch.zeros(1, 1, 1, 1, device=dev()),
                torch.zeros(4, 4, device=dev()), torch.zeros(1, 1, 4, 4, 4, device=dev()),
                torch.zeros(0, 4, 4, 4, device=dev())):
        with pytest.raises(ValueError):
            voxel_mesh(bad)
    with pytest.raises(ValueError):
        voxel_mesh(ok, threshold=float('nan'))
    with pytest.raises(ValueError):
        voxel_mesh(ok.cpu().numpy())
    oc, depth = octree('random5')
    for bad in (0, -1, depth + 1):
        with pytest.raises(ValueError):
            octree_mesh(oc, bad)
    v, f = voxel_mesh(ok)[0]
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)


CFG3 = dict(image_size=[8, 32, 128], input_depth=[3, 5, 7], unet_type=['lr', 'hr', 'feature'], full_depth=3,
            input_channels=[8, 8, 3], out_channels=[8, 8, 3], model_channels=[16, 32, 32],
            num_res_blocks=[[1, 1, 1], [1, 1, 0], [1, 1, 1]], attention_resolutions=[2, 4],
            channel_mult=[[1, 2, 4], [1, 2, 4], [1, 2, 4]], num_heads=4, use_checkpoint=False, dims=3,
            df_type=['x0', 'x0', 'x0'])


def same(a, b):
    assert len(a) == len(b)
    for (va, fa), (vb, fb) in zip(a, b):
        assert torch.equal(va, vb) and torch.equal(fa, fb)


def test_pipeline_adds_the_octree_meshes():
    from octfusion_amd import pipeline, synthetic
    from octfusion_amd.graph_unet_union import UNet3DModel
    net = UNet3DModel(**{k: v for k, v in dict(CFG3, stage_flag='feature').items() if k != 'df_type'})
    net.load_state_dict(synthetic.random_state_dict(net))
    net = net.to(dev()).eval()
    cs = pipeline.CascadeSampler(net, CFG3, None)
    split = C.random_split_small(2, 3, 4).to(dev())
    out = cs.sample(2, ddim_steps=2, seed=7, split_small=split, use_graph=False, octree_mesh=True)
    assert len(out['octree_meshes']) == 2 and len(out['octree_meshes_large']) == 2
    same(out['octree_meshes'], octree_mesh(out['octree_small'], 5))
    same(out['octree_meshes_large'], octree_mesh(out['octree_large'], 7))
    assert all(f.shape[0] > 0 for _, f in out['octree_meshes'])
    # two stages: the small depth only; without the flag no key
    cfg2 = dict(CFG3, unet_type=['lr', 'hr'], input_depth=[3, 5], df_type=['x0', 'x0'])
    cs2 = pipeline.CascadeSampler(net, cfg2, None)
    out2 = cs2.sample(2, ddim_steps=2, seed=7, split_small=split, use_graph=False, octree_mesh=True)
    same(out2['octree_meshes'], out['octree_meshes'])
    assert 'octree_meshes_large' not in out2
    plain = cs2.sample(2, ddim_steps=2, seed=7, split_small=split, use_graph=False)
    assert 'octree_meshes' not in plain and 'octree_meshes_large' not in plain
    assert sorted(plain) == sorted(k for k in out2 if k != 'octree_meshes')


def test_write_outputs_puts_the_octree_meshes_in_their_folders(tmp_path):
    from octfusion_amd import generate as G, mesh
    oc, depth = octree('random5')
    meshes = octree_mesh(oc, depth)
    coarse = octree_mesh(oc, depth - 1)
    out = {'octree_small': oc, 'octree_meshes': meshes, 'octree_meshes_large': coarse}
    G.write_outputs(str(tmp_path), [4, 9], {k: v for k, v in out.items()}, dict(full_depth=3, input_depth=[3, 5]))
    for b, i in enumerate([4, 9]):
        for sub, ms in (('octree', meshes), ('octree_large', coarse)):
            v, f = mesh.read_obj(os.path.join(str(tmp_path), sub, '%d.obj' % i))
            assert np.array_equal(v, host(ms[b])[0]) and np.array_equal(f, host(ms[b])[1])
