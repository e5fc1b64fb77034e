"""GPU tests of the mesh checker (csrc/ofx_meshcheck.hip; mesh_check.weld / check, mesh_to_sdf(signed='auto'), the
command lines) against the float64 oracle (tests/meshcheck_oracle.py) on the meshes of tests/meshcheck_cases.py.
tests/test_meshcheck_oracle.py pins that oracle to hand-written answers on the CPU.

What must be equal: every integer -- rep, index, the welded faces, all counts, edge_faces, partners, first, pairs.
area and volume: |device - oracle| <= 1e-10 x the sum of the absolute terms (the fp64 summation error of F <= 2^20
terms is below F 2^-53 = 1.2e-10 of that sum, whatever the order); the deviation is printed.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import meshcheck_cases as C
import meshcheck_oracle as MO

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_KEYS = list(MO.K_COUNTS)


def dev():
    return torch.device('cuda:0')


def to_dev(m):
    v, f = m
    return (torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev()),
            torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(dev()))


def run(meshes, **kw):
    """check(weld=False, detail=True) on numpy meshes -> one dict per mesh with numpy per-face arrays."""
    from octfusion_amd import mesh_check as MC
    kw.setdefault('weld', False)
    out = MC.check([to_dev(m) for m in meshes], detail=True, **kw)
    assert len(out) == len(meshes)
    for r in out:
        for k in ('edge_faces', 'partners', 'first'):
            r[k] = r[k].cpu().numpy()
    return out


_oracle = {}


def oracle(name, m):
    """The oracle's report of a mesh, computed once per name and never changed."""
    if name not in _oracle:
        v, f = m
        t = MO.topology(v, f)
        partners, first, pairs = MO.selfx(v, f)
        t.update(partners=partners, first=first, self_intersections=pairs)
        t.update(MO.derived(t, len(f), len(v)))
        _oracle[name] = t
    return _oracle[name]


def assert_same(name, r, o):
    for k in INT_KEYS + ['self_intersections', 'euler', 'genus', 'closed', 'edge_manifold', 'oriented', 'watertight']:
        assert r[k] == o[k], (name, k, r[k], o[k])
    for k in ('edge_faces', 'partners', 'first'):
        assert r[k].shape == o[k].shape and np.array_equal(r[k], o[k]), (name, k)
    for k in ('area', 'volume'):
        err, scale = abs(r[k] - o[k]), o[k + '_abs']
        print('%s: %s %.17g, |device - oracle| = %.3e = %.2e of the sum of |terms|'
              % (name, k, r[k], err, err / scale if scale else 0.0))
        assert err <= 1e-10 * scale


def same_report(a, b):
    """Bitwise: every field of two device reports, the fp64 sums by their bits."""
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        elif isinstance(a[k], float):
            assert np.float64(a[k]).view(np.int64) == np.float64(b[k]).view(np.int64), k
        else:
            assert a[k] == b[k], k


@pytest.fixture(scope='module')
def general():
    return C.general()


@pytest.fixture(scope='module')
def general_results(general):
    """The device reports of the general shapes from ONE batched call (shared, never changed)."""
    return run([m for _, m in general])


# ---- 1 values -----------------------------------------------------------------------------------------------------
def test_planted_cases_in_one_batch():
    pairs = C.pairs()
    more = [('cube soup', C.unwelded(C.cube(2.0))), ('cube', C.cube(2.0)), ('flipped', C.cube_one_face_flipped()),
            ('removed', C.cube_one_face_removed()), ('two cubes, unwelded', C.two_cubes_sharing_an_edge())]
    meshes = [(p[1], p[2]) for p in pairs] + [m for _, m in more]
    res = run(meshes)
    for (name, v, f, hit, dup), r in zip(pairs, res):
        assert r['self_intersections'] == (1 if hit else 0), name           # the hand-written answer
        assert r['partners'].tolist() == ([1, 1] if hit else [0, 0]), name
        assert r['first'].tolist() == ([1, 0] if hit else [-1, -1]), name
        assert r['duplicate_faces'] == dup, name
        assert_same(name, r, oracle(name, (v, f)))
    for (name, m), r in zip(more, res[len(pairs):]):
        assert_same(name, r, oracle(name, m))
    cube = res[len(pairs) + 1]
    assert cube['edges'] == 18 and cube['euler'] == 2 and cube['genus'] == 0 and cube['watertight']
    assert cube['self_intersections'] == 0 and cube['area'] == 24.0 and abs(cube['volume'] - 8.0) < 1e-12
    assert res[len(pairs)]['components'] == 12 and res[len(pairs)]['self_intersections'] > 0
    assert res[len(pairs) + 2]['inconsistent_edges'] == 3 and res[len(pairs) + 3]['boundary_edges'] == 3


def test_general_shapes_in_one_batch(general, general_results):
    for (name, m), r in zip(general, general_results):
        o = oracle(name, m)
        print(name, len(m[1]), 'faces', {k: r[k] for k in INT_KEYS}, 'pairs', r['self_intersections'])
        assert_same(name, r, o)
    by = dict(zip([n for n, _ in general], general_results))
    assert [by[n]['self_intersections'] for n in ('sphere', 'torus', 'open', 'soup')] == [0, 0, 0, 229]
    assert by['random_signs']['nonmanifold_edges'] == 6 and by['random_signs']['faces'] == 3340
    assert by['simplified_torus']['nonmanifold_edges'] == 8


def test_strips_across_the_wave_and_staging_boundaries():
    sizes = [1, 2, 63, 64, 65, 129]
    meshes = [C.strip(n) for n in sizes]
    for n, m, r in zip(sizes, meshes, run(meshes)):
        assert r['faces'] == n
        assert_same('strip %d' % n, r, oracle('strip %d' % n, m))


def test_one_bin_many_staging_rounds(general, general_results):
    sphere = general[0][1]
    assert general[0][0] == 'sphere' and len(sphere[1]) == 1280
    same_report(run([sphere], bins=1)[0], general_results[0])


def test_a_one_face_shape_between_two_large_ones(general, general_results):
    one = C.strip(1)
    res = run([general[3][1], one, general[4][1]])
    same_report(res[0], general_results[3])
    same_report(res[2], general_results[4])
    assert_same('strip 1', res[1], oracle('strip 1', one))


# ---- 2 weld -------------------------------------------------------------------------------------------------------
def weld_meshes():
    nan = float('nan')
    v = np.array([[1, 2, 3], [0.0, 0, 0], [1, 2, 3], [-0.0, 0, -0.0], [nan, 0, 0], [nan, 0, 0], [1, 2, 3.0000002]],
                 np.float32)
    f = np.array([[0, 1, 2], [3, 2, 6]], np.int32)
    rng = np.random.default_rng(3)
    sv, sf = C.unwelded(C.general()[0][1])                 # the sphere as a soup, its faces shuffled
    sf = sf[rng.permutation(len(sf))]
    return [(v, f), C.unwelded(C.cube(2.0)), C.two_cubes_sharing_an_edge(), (sv, sf), C.strip(1)]


def test_weld_equals_the_oracle():
    from octfusion_amd import mesh_check as MC
    meshes = weld_meshes()
    g = MC._gather([to_dev(m) for m in meshes], 'test')
    _, _, rep = MC._weld(g, 'test')
    reps = [r.cpu().numpy() for r in rep.split(g['nv'])]
    out = MC.weld([to_dev(m) for m in meshes])
    alone = MC.weld([to_dev(meshes[3])])[0]
    for k, (m, (v, f, index)) in enumerate(zip(meshes, out)):
        orep, ov, of, oindex = MO.weld(*m)
        assert np.array_equal(reps[k], orep), k
        assert np.array_equal(index.cpu().numpy(), oindex), k
        assert np.array_equal(f.cpu().numpy(), of), k
        assert np.array_equal(v.cpu().numpy().view(np.uint32), ov.view(np.uint32)), k
    assert out[1][0].shape[0] == 8 and out[2][0].shape[0] == 14 and out[0][0].shape[0] == 5
    for a, b in zip(alone, out[3]):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_check_welds_first_by_default():
    from octfusion_amd import mesh_check as MC
    soup, two = to_dev(C.unwelded(C.cube(2.0))), to_dev(C.two_cubes_sharing_an_edge())
    r, t = MC.check([soup, two])
    assert (r['vertices'], r['welded_vertices'], r['edges'], r['euler'], r['genus']) == (8, 28, 18, 2, 0)
    assert r['watertight'] and r['oriented'] and r['self_intersections'] == 0 and r['components'] == 1
    assert r['area'] == 24.0 and abs(r['volume'] - 8.0) < 1e-12
    assert t['vertices'] == 14 and t['nonmanifold_edges'] == 1 and not t['watertight'] and t['genus'] is None
    raw = MC.check([soup], weld=False, intersections=False)[0]
    assert raw['components'] == 12 and raw['welded_vertices'] == 0 and raw['self_intersections'] is None
    assert 'edge_faces' not in raw


# ---- 3 purity -----------------------------------------------------------------------------------------------------
def test_batch_bins_and_run_do_not_change_a_bit(general, general_results):
    meshes = [m for _, m in general]
    for k in (0, 3, 4):
        same_report(run([meshes[k]])[0], general_results[k])                # alone against batched
    for bins in (1, 4, 16, 0):
        for a, b in zip(run(meshes[2:5], bins=bins), general_results[2:5]):
            same_report(a, b)
    for a, b in zip(run(meshes), general_results):                           # a second run
        same_report(a, b)


def test_a_permutation_of_the_faces(general, general_results):
    name, (v, f) = general[3]
    base = general_results[3]
    assert name == 'soup' and base['self_intersections'] == 229
    perm = np.random.default_rng(11).permutation(len(f))
    inv = np.argsort(perm)
    r = run([(v, f[perm])])[0]
    assert np.array_equal(r['partners'], base['partners'][perm])
    assert np.array_equal(r['edge_faces'], base['edge_faces'][perm])
    one = base['partners'][perm] == 1                    # a single partner: first is that face, wherever it went
    assert one.sum() > 50 and np.array_equal(r['first'][one], inv[base['first'][perm][one]])
    o = MO.selfx(v, f[perm])                             # several: the lowest of them in the new numbering
    assert np.array_equal(r['first'], o[1]) and r['self_intersections'] == o[2] == 229
    for k in INT_KEYS:
        assert r[k] == base[k], k


# ---- 4 errors -----------------------------------------------------------------------------------------------------
def test_bad_meshes_are_refused_by_name():
    from octfusion_amd import mesh_check as MC
    good = [C.cube(2.0), C.strip(65)]
    want = run(good)
    v, f = C.cube(2.0)
    bad_index = (v, np.concatenate([f, [[0, 1, 8]]]).astype(np.int32))
    nan_used = (np.where(np.arange(8)[:, None] == 5, np.float32('nan'), v).astype(np.float32), f)
    for bad in (bad_index, nan_used):
        for fn in (lambda ms: MC.check(ms), lambda ms: MC.check(ms, weld=False), lambda ms: MC.weld(ms)):
            with pytest.raises(ValueError, match='shape 1 '):
                fn([to_dev(good[0]), to_dev(bad), to_dev(good[1])])
        for a, b in zip(run(good), want):                                    # the others, in a call without it
            same_report(a, b)
    with pytest.raises(ValueError, match='shape 1 has no faces'):
        MC.check([to_dev(good[0]), (to_dev(good[0])[0], torch.zeros(0, 3, dtype=torch.int32, device=dev()))])
    with pytest.raises(ValueError, match='bins'):
        MC.check([to_dev(good[0])], bins=17)


def test_an_unused_nan_vertex_is_unreferenced_and_never_welded():
    from octfusion_amd import mesh_check as MC
    v, f = C.cube(2.0)
    nan = np.full((2, 3), np.nan, np.float32)
    m = (np.concatenate([v, nan, v[:1]]), f)
    vw, fw, index = MC.weld([to_dev(m)])[0]
    assert index.cpu().tolist() == list(range(10)) + [0]
    assert vw.shape[0] == 10 and torch.isnan(vw[8:]).all()
    r = MC.check([to_dev(m)])[0]
    assert r['unreferenced_vertices'] == 2 and r['welded_vertices'] == 1 and r['watertight'] and r['euler'] == 2
    assert_same('nan cube', run([m])[0], oracle('nan cube', m))


def test_entry_points_refuse_bad_arguments():
    from octfusion_amd import _lib
    L = _lib.lib()
    assert L.ofx_mesh_weld_ws_bytes(0, 8, 12) == 0 and L.ofx_mesh_weld_ws_bytes(1, 0, 12) == 0
    assert L.ofx_mesh_weld_ws_bytes(1, 2 ** 30 + 1, 12) == 0 and L.ofx_mesh_weld_ws_bytes(65536, 8, 12) == 0
    assert L.ofx_mesh_topology_ws_bytes(1, 8, 0) == 0 and L.ofx_mesh_topology_ws_bytes(1, 8, 2 ** 30 // 3 + 1) == 0
    assert L.ofx_mesh_selfx_ws_bytes(1, 8, 12, 17) == 0 and L.ofx_mesh_selfx_ws_bytes(1, 8, 12, -1) == 0
    assert L.ofx_mesh_weld_ws_bytes(1, 8, 12) > 0 and L.ofx_mesh_topology_ws_bytes(1, 8, 12) > 0
    assert L.ofx_mesh_selfx_ws_bytes(1, 8, 12, 0) > 0
    v, f = to_dev(C.cube(2.0))
    offs = torch.tensor([[0, 8], [0, 12]], dtype=torch.int64, device=dev())
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev())
    sentinel = torch.full((64,), -77, dtype=torch.int32, device=dev())
    s = sentinel.clone()
    p = _lib.ptr
    mesh_args = (p(v), p(f), p(offs[0]), p(offs[1]))
    assert L.ofx_mesh_weld(*mesh_args, 0, 8, 12, p(s), p(s), p(ws), p(s), None) == -1
    assert L.ofx_mesh_weld(*mesh_args, 1, 8, 12, None, p(s), p(ws), p(s), None) == -1
    assert L.ofx_mesh_topology(*mesh_args, 1, 8, 0, p(s), p(s), None, p(ws), p(s), None) == -1
    assert L.ofx_mesh_selfx(*mesh_args, 1, 12, 17, p(s), p(s), p(s), p(ws), p(s), None) == -1
    assert L.ofx_mesh_selfx(*mesh_args, 1, 0, 0, p(s), p(s), p(s), p(ws), p(s), None) == -1
    torch.cuda.synchronize()
    assert torch.equal(s, sentinel)


# ---- 5 the sign rule ----------------------------------------------------------------------------------------------
def test_signed_auto_takes_the_rule_the_check_finds(general):
    from octfusion_amd import mesh2sdf as M
    meshes = [to_dev(m) for _, m in general[:4]]
    stats = {}
    auto = M.mesh_to_sdf(meshes, 16, signed='auto', stats=stats)
    assert stats['sign'] == ['parity', 'parity', 'winding', 'winding']
    assert [r['watertight'] for r in stats['check']] == [True, True, False, False]
    parity = M.mesh_to_sdf(meshes[:2], 16, signed=True)
    winding = M.mesh_to_sdf(meshes[2:], 16, signed='winding')
    assert torch.equal(auto[:2].view(torch.int32), parity.view(torch.int32))
    assert torch.equal(auto[2:].view(torch.int32), winding.view(torch.int32))
    st = {}
    one = M.compute(*general[2][1], size=16, sign='auto', stats=st)
    assert st['sign'] == ['winding'] and torch.equal(one.view(torch.int32), winding[0].view(torch.int32))
    with pytest.raises(ValueError):
        M.mesh_to_sdf(meshes[:1], 16, signed='other')


# ---- 6 command lines ----------------------------------------------------------------------------------------------
def _child(args, **kw):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable] + args, capture_output=True, text=True, cwd=ROOT, env=env, **kw)
    assert out.returncode == 0, out.stderr[-2000:]
    return [json.loads(l) for l in out.stdout.splitlines() if l.startswith('{')]


def test_mesh_check_command_line(tmp_path):
    from octfusion_amd import mesh
    a, b, c = str(tmp_path / 'cube.obj'), str(tmp_path / 'open.obj'), str(tmp_path / 'bad.obj')
    mesh.write_obj(a, *C.unwelded(C.cube(2.0)))
    mesh.write_obj(b, *C.cube_one_face_removed())
    with open(c, 'w') as fh:
        fh.write('v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 9\n')
    rows = _child(['-m', 'octfusion_amd.mesh_check', '--input', a, b, c, '--json', str(tmp_path / 'r.json')])
    assert [r['name'] for r in rows] == [a, b, c]
    assert rows[0]['watertight'] and rows[0]['vertices'] == 8 and rows[0]['genus'] == 0
    assert rows[0]['self_intersections'] == 0
    assert rows[1]['boundary_edges'] == 3 and not rows[1]['closed']
    assert 'error' in rows[2]                                              # reported, and the exit status is still 0
    assert json.load(open(str(tmp_path / 'r.json'))) == rows
    raw = _child(['-m', 'octfusion_amd.mesh_check', '--input', a, '--no-weld', '--no-intersections'])
    assert raw[0]['components'] == 12 and raw[0]['self_intersections'] is None


def test_simplify_command_line_reports_its_outputs(tmp_path):
    import mc_oracle as M
    from octfusion_amd import mesh
    src = str(tmp_path / 'torus.obj')
    mesh.write_obj(src, *M.marching_cubes(M.torus(32)))
    rows = _child(['-m', 'octfusion_amd.simplify', '--input', src, '--out', str(tmp_path / 'out'), '--cells', '10',
                   '--check'])
    assert len(rows) == 2 and rows[0]['name'] == 'torus' and rows[1]['check'] == [rows[0]]
    assert rows[0]['nonmanifold_edges'] == 8 and not rows[0]['watertight']  # what the clean torus turns into


GENERATE = """
import sys
from octfusion_amd import configs, generate, mesh
configs.CONFIGS['tiny_uncond'] = dict(configs.SNET_UNCOND, model_channels=[32, 32])
configs.VAES['tiny_uncond'] = configs.VAES['snet_uncond']
mesh.MESH_SCALES['tiny_uncond'] = mesh.MESH_SCALES['snet_uncond']
generate.main(['--config', 'tiny_uncond', '--shapes', '1', '--steps', '2', '--batch', '1', '--sdf-resolution', '32',
               '--seed', '5', '--mesh', '--check', '--out', sys.argv[1]])
"""


def test_generate_command_line_writes_the_reports(tmp_path):
    from octfusion_amd import mesh
    out = str(tmp_path / 'gen')
    line = _child(['-c', GENERATE, out])[-1]
    saved = json.load(open(os.path.join(out, 'mesh_check.json')))
    assert saved == line['rank0_mesh_check'] and len(saved) == 1 and saved[0]['name'] == '0.obj'
    if line['rank0_mesh_faces'][0]:
        v, f = mesh.read_obj(os.path.join(out, '0.obj'))
        assert saved[0]['faces'] == len(f) and saved[0]['boundary_edges'] >= 0
    else:
        assert 'error' in saved[0]
