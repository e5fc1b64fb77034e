"""Mesh simplification on the device (csrc/ofx_simplify.hip through octfusion_amd.simplify) against the numpy oracle
(tests/simplify_oracle.py).

Compared exactly: faces, the four stats, dtypes, the vertex count.  Vertices: |got - want| <= one fp32 ulp at the mesh's
largest input coordinate, absolute, `want` being the oracle's float64 position rounded to fp32.  Why one ulp: the fp64
sums of the two sides differ by summation order, about n 2^-53 relative; the solve amplifies that by at most its
condition number 3 / reg + 1 = 3001; so the float64 positions differ by orders of magnitude less than half an fp32 ulp
and their roundings by at most one ulp at the coordinate's magnitude, which the largest coordinate bounds.  Every
coordinate is compared."""
import json
import os

import numpy as np
import pytest
import torch

import mc_oracle as M
import simplify_oracle as S

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def dev():
    return torch.device('cuda:0')


def mc(fields, **kw):
    from octfusion_amd import mesh
    return mesh.marching_cubes(torch.from_numpy(np.stack(fields)).to(dev()), **kw)


def to_dev(v, f):
    return (torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev()),
            torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(dev()))


def host(m):
    return m[0].cpu().numpy(), m[1].cpu().numpy()


def check(meshes, **kw):
    """Simplify on the device and compare every mesh with the oracle; returns (outputs, stats, oracle stats)."""
    from octfusion_amd import simplify
    stats = {}
    got = simplify.simplify(meshes, stats=stats, **kw)
    assert len(got) == len(meshes) and len(stats['meshes']) == len(meshes)
    want_stats = []
    for k, (m, g) in enumerate(zip(meshes, got)):
        v, f = host(m)
        wv, wf, wst = S.simplify(v, f, **kw)
        gv, gf = host(g)
        assert g[0].dtype == torch.float32 and g[1].dtype == torch.int32
        assert g[0].device == m[0].device and g[1].device == m[1].device
        assert stats['meshes'][k] == wst, k
        assert all(type(x) is int for x in stats['meshes'][k].values())
        assert gv.shape == wv.shape and gf.shape == wf.shape, k
        assert np.array_equal(gf, wf), k
        if len(wv):
            tol = np.spacing(np.float32(np.abs(v).max()))
            err = np.abs(gv.astype(np.float64) - wv.astype(np.float64)).max()
            print('mesh %d: %d -> %d faces, max vertex error %.3g (bound %.3g)' % (k, len(f), len(wf), err, tol))
            assert err <= tol, (k, err, tol)
        want_stats.append(wst)
    return got, stats['meshes'], want_stats


@pytest.fixture(scope='module')
def sphere32():
    return mc([M.sphere(32)])[0]


@pytest.mark.parametrize('cells', [1, 2, 5, 13])
def test_sphere_cells(sphere32, cells):
    got, st, _ = check([sphere32], cells=cells)
    v, f = host(got[0])
    if cells == 1:
        assert len(v) == 0 and len(f) == 0 and st[0]['clusters'] == 1 and st[0]['clusters_unused'] == 1
        return
    if cells == 2:                               # eight clusters, hundreds of incident faces each: the wave loop
        assert st[0]['clusters'] == 8 and int(sphere32[1].shape[0]) // 8 > 64 * 4
    assert M.directed_edge_balance(f) and M.euler(v, f) == 2


def test_cell_size_mode(sphere32):
    got, st, _ = check([sphere32], cell_size=3 * 1.8 / 32)
    v, f = host(got[0])
    assert len(f) > 100 and M.directed_edge_balance(f) and M.euler(v, f) == 2


@pytest.mark.parametrize('cells', [4, 8])
def test_random_signs_duplicates_and_unused_clusters(cells):
    """Duplicate faces, clusters no face uses, non-manifold input.  The oracle's figures for random_signs(12) under the
    rule as stated (vertices at the box's upper faces clamped into the last cell): cells = 4 gives 14 duplicates and 0
    unused clusters (all 64 cells are used), cells = 8 gives 3 and 9.  The 8 / 5 and 3 / 10 of the prototype came from
    a grid without that clamp; `cell_size = side / cells` lays exactly that grid (an extra layer of cells at the upper
    faces), so those two cases run here as well and reproduce its figures.  Every case must exercise the duplicate
    path; every case but cells = 4 the unused-cluster path too."""
    m = mc([M.random_signs(12)])[0]
    v, f = host(m)
    side = float((v.max(0).astype(np.float64) - v.min(0).astype(np.float64)).max())
    proto = {4: (8, 5), 8: (3, 10)}[cells]
    for kw in (dict(cells=cells), dict(cell_size=side / cells)):
        wst = S.simplify(v, f, **kw)[2]
        print(kw, wst)
        assert wst['faces_duplicate'] > 0
        if 'cell_size' in kw:
            assert (wst['faces_duplicate'], wst['clusters_unused']) == proto
        if kw != dict(cells=4):
            assert wst['clusters_unused'] > 0
        check([m], **kw)


def test_ragged_batch_is_bitwise_the_single_meshes():
    from octfusion_amd import simplify
    a = mc([M.sphere(16)])[0]
    b = to_dev(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.zeros((0, 3), np.int32))
    c = mc([M.random_signs(12)])[0]
    d = mc([M.torus(24)])[0]
    batch = [a, b, c, d]
    got, st, _ = check(batch, cells=6)
    assert got[1][0].shape[0] == 0 and got[1][1].shape[0] == 0
    assert st[1] == dict(clusters=0, faces_collapsed=0, faces_duplicate=0, clusters_unused=0)
    again = simplify.simplify(batch, cells=6)
    for k, m in enumerate(batch):
        s1 = {}
        one = simplify.simplify([m], cells=6, stats=s1)[0]
        assert s1['meshes'][0] == st[k]
        for x, y, z in zip(got[k], one, again[k]):
            assert x.dtype == y.dtype and torch.equal(x, y) and torch.equal(x, z), k
            if x.dtype == torch.float32:
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), k
                assert torch.equal(x.view(torch.int32), z.view(torch.int32)), k


def plane_mesh():
    """A 5 x 5 planar grid of integer vertices (z = 0), two triangles per square; then an unreferenced vertex far
    outside (it moves lo / hi), a face with a repeated index, and three collinear vertices in three cells of their own
    joined by one face."""
    g = np.array([[x, y, 0] for x in range(5) for y in range(5)], np.float32)
    f = []
    for x in range(4):
        for y in range(4):
            p = x * 5 + y
            f += [[p, p + 5, p + 6], [p, p + 6, p + 1]]
    v = np.concatenate([g, [[-6, -4, 10]], [[20, 0, 0], [24, 0, 0], [28, 0, 0]]]).astype(np.float32)
    f += [[0, 0, 1], [26, 27, 28]]
    return v, np.array(f, np.int32)


def test_hand_built_plane():
    v, f = plane_mesh()
    d = {}
    wv, wf, wst = S.simplify(v, f, cell_size=2.0, detail=d)
    # the collinear face is kept, adds nothing, and its clusters sit at their (single) input vertices
    assert wf.tolist()[-1] == [len(wv) - 3, len(wv) - 2, len(wv) - 1]
    assert np.array_equal(wv[-3:], v[26:29])
    assert wst['clusters_unused'] == 1                     # the far vertex's cell
    assert wst['faces_collapsed'] >= 1 + 8                 # the repeated index, and faces inside one cell
    assert (wv[:-3, 2] == 0).all()
    got, st, _ = check([to_dev(v, f)], cell_size=2.0)
    assert np.array_equal(host(got[0])[0][-3:], v[26:29])


def test_shift_and_scale(sphere32):
    v, f = host(sphere32)
    big = (v.astype(np.float64) * 20 + np.array([37.0, -5.0, 11.0])).astype(np.float32)
    check([to_dev(big, f)], cells=5)
    check([to_dev(big, f)], cell_size=20 * 3 * 1.8 / 32)


def test_larger_sphere():
    m = mc([M.sphere(64)])[0]
    assert int(m[1].shape[0]) == 11912                     # > 2^13 faces, 1010 clusters: several blocks everywhere
    got, _, _ = check([m], cells=16)
    v, f = host(got[0])
    assert M.directed_edge_balance(f) and M.euler(v, f) == 2


def test_errors(sphere32):
    from octfusion_amd import simplify
    dv, df = sphere32
    for kw in (dict(), dict(cells=4, cell_size=0.1), dict(cells=0), dict(cells=1025), dict(cells=2.5),
               dict(cell_size=0.0), dict(cell_size=-1.0), dict(cell_size=float('inf')), dict(cell_size=float('nan')),
               dict(cells=4, reg=0.0), dict(cells=4, reg=1.5), dict(cells=4, reg=float('nan'))):
        with pytest.raises(ValueError):
            simplify.simplify([(dv, df)], **kw)
    for bad in ((dv, df.long()), (dv.double(), df), (dv.cpu(), df.cpu()), (dv, df.cpu())):
        with pytest.raises(ValueError):
            simplify.simplify([bad], cells=4)
    hi = df.clone()
    hi[7, 1] = dv.shape[0]                                 # == V
    lo = df.clone()
    lo[0, 0] = -1
    for b in (hi, lo):
        with pytest.raises(ValueError, match='shape 1 has a face index'):
            simplify.simplify([(dv, df), (dv, b)], cells=4)
    with pytest.raises(ValueError, match='shape 2 needs 1024 or more cells'):
        simplify.simplify([(dv, df), (dv, df), (dv * 2, df)], cell_size=1.2 / 1024)      # sides ~ 1, 1 and 2
    check([(dv, df)], cell_size=1.2 / 1024)                # the same grid fits the unit sphere: ~ 854 cells a side
    check([(dv, df)], cells=4)                              # and a good call after the bad ones is clean


def test_cli_round_trip(tmp_path, capsys, sphere32):
    from octfusion_amd import mesh, simplify
    v, f = host(sphere32)
    mesh.write_obj(str(tmp_path / 'in' / 'ball.obj'), v, f)
    res = simplify.main(['--input', str(tmp_path / 'in'), '--out', str(tmp_path / 'out'), '--cells', '5'])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1]
    assert json.loads(line) == res
    wv, wf, wst = S.simplify(*mesh.read_obj(str(tmp_path / 'in' / 'ball.obj')), cells=5)
    gv, gf = mesh.read_obj(str(tmp_path / 'out' / 'ball.obj'))
    assert np.array_equal(gf, wf) and np.abs(gv - wv).max() <= np.spacing(np.float32(np.abs(v).max()))
    assert res['faces_in'] == [len(f)] and res['faces_out'] == [len(wf)] and res['stats'] == [wst]


def _tiny():
    from octfusion_amd import configs, mesh
    configs.CONFIGS['tiny_uncond'] = dict(configs.SNET_UNCOND, model_channels=[32, 32])
    configs.VAES['tiny_uncond'] = configs.VAES['snet_uncond']
    mesh.MESH_SCALES['tiny_uncond'] = mesh.MESH_SCALES['snet_uncond']


def test_generate_cli_simplify(tmp_path):
    """`--mesh --simplify 8` writes the simplified mesh as <index>.obj, and without the flag nothing changes."""
    from octfusion_amd import generate as G, mesh, simplify
    _tiny()
    base = ['--config', 'tiny_uncond', '--shapes', '2', '--steps', '4', '--batch', '2', '--sdf-resolution', '64',
            '--seed', '5', '--mesh']
    plain = G.main(base + ['--out', str(tmp_path / 'plain')])
    res = G.main(base + ['--simplify', '8', '--out', str(tmp_path / 'simple')])
    assert 'rank0_simple_faces' not in plain and 'rank0_simple_vertices' not in plain
    drop = ('seconds_max_over_ranks', 'seconds_per_shape', 'shapes_per_s', 'rank0_phase_seconds')
    assert {k: x for k, x in plain.items() if k not in drop} == \
        {k: x for k, x in res.items() if k not in drop + ('rank0_simple_vertices', 'rank0_simple_faces')}
    written = 0
    for k, i in enumerate(res['rank0_indices']):
        sdf = torch.load(os.path.join(str(tmp_path / 'simple'), str(i), 'sdf.pt'))
        assert torch.equal(sdf, torch.load(os.path.join(str(tmp_path / 'plain'), str(i), 'sdf.pt')))
        full = mesh.marching_cubes(sdf[None].to(dev()), scale=0.5)
        assert (res['rank0_mesh_vertices'][k], res['rank0_mesh_faces'][k]) == \
            (int(full[0][0].shape[0]), int(full[0][1].shape[0]))
        sv, sf = host(simplify.simplify(full, cells=8)[0])
        assert (res['rank0_simple_vertices'][k], res['rank0_simple_faces'][k]) == (len(sv), len(sf))
        p_plain = os.path.join(str(tmp_path / 'plain'), '%d.obj' % i)
        p_simple = os.path.join(str(tmp_path / 'simple'), '%d.obj' % i)
        if full[0][1].shape[0]:
            v, f = mesh.read_obj(p_plain)                   # the run without the flag still writes the full mesh
            assert np.array_equal(f, host(full[0])[1]) and np.array_equal(v, host(full[0])[0])
        if len(sf) == 0:
            assert not os.path.exists(p_simple)
            continue
        v, f = mesh.read_obj(p_simple)
        assert np.array_equal(f, sf) and np.array_equal(v, sv)
        written += 1
    assert written > 0
    with pytest.raises(ValueError, match='--simplify needs --mesh'):
        G.main(['--config', 'tiny_uncond', '--shapes', '1', '--simplify', '8'])
