"""GPU tests of the winding numbers (csrc/ofx_winding.hip; mesh_query.winding_number / occupancy, the 'winding' sign
of closest_point, mesh_error, mesh_to_sdf and compute) against the float64 oracle (tests/winding_oracle.py).

Shapes and query sets: winding_oracle.shapes() / query_sets() -- icosphere(3) 1280 faces, torus(32, 16) 1024, that
sphere with its cap cut off 1040, a soup of two overlapping spheres, a box and a plate 2574, a plate 2; 4096 queries
each.  tests/test_winding_oracle.py establishes on the CPU what these tests lean on and prints the numbers.

Tolerances.
  exact   |w - oracle| <= 1e-6: four fp32 half-ulps at |w| <= 4 (the result is rounded to fp32 once); the fp64 sum of
          at most 2574 terms of size <= 1/2 is six orders below that.  Queries within 1e-5 of their mesh are left
          out (there atan2 sits on its jump), at most 0.1 % of a set.
  far     (a) against the restated far field, where the restatement's near / far decisions have a margin above 1e-9,
          the same 1e-6: the same arithmetic up to the order of sums.  (b) against the exact oracle 2 E + 1e-6 and (c)
          the same side of 0.5 wherever |w_exact - 0.5| > 2 E, E = the restatement's own largest error for that shape
          and setting, computed here by the oracle; the factor 2 because a borderline bin may fall on the other side.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh2sdf_oracle as O
import meshquery_oracle as Q
import winding_oracle as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['sphere', 'torus', 'open', 'soup', 'plate']
TOL = 1e-6


def dev():
    return torch.device('cuda:0')


def to_dev(m):
    v, f = m
    return (torch.from_numpy(np.asarray(v, np.float32)).to(dev()), torch.from_numpy(np.asarray(f, np.int32)).to(dev()))


def pts_dev(P):
    return torch.from_numpy(np.ascontiguousarray(P, np.float32)).to(dev())


def run(meshes, sets, **kw):
    """winding_number on numpy meshes and query sets -> per mesh w fp32, numpy."""
    from octfusion_amd import mesh_query as MQ
    out = MQ.winding_number([to_dev(m) for m in meshes], [pts_dev(P) for P in sets], **kw)
    assert len(out) == len(meshes)
    for w, P in zip(out, sets):
        assert w.shape == (len(P),) and w.dtype == torch.float32
    return [w.cpu().numpy() for w in out]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.fixture(scope='module')
def cases():
    meshes = W.shapes()
    assert [n for n, _ in meshes] == NAMES
    assert [len(m[1]) for _, m in meshes] == [1280, 1024, 1040, 2574, 2]
    sets = W.query_sets([m for _, m in meshes])
    out = {}
    for (name, m), P in zip(meshes, sets):
        out[name] = {'mesh': m, 'P': P, 'w': W.exact(P, *m), 'd': Q.query(P, *m)[0]}
    return out


@pytest.fixture(scope='module')
def results(cases):
    """The exact device values of the five shapes from ONE batched call (shared, never changed)."""
    return dict(zip(NAMES, run([cases[n]['mesh'] for n in NAMES], [cases[n]['P'] for n in NAMES])))


_far_oracle = {}


def far_oracle(cases, name, bins, beta):
    """(w_restated, margin, E) of a shape at a far-field setting, computed once."""
    key = (name, bins, beta)
    if key not in _far_oracle:
        c = cases[name]
        wf, margin, _ = W.far(c['P'], *c['mesh'], bins, beta)
        _far_oracle[key] = (wf, margin, float(np.abs(wf - c['w']).max()))
    return _far_oracle[key]


# ---- 1 exact values -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_exact_values(name, cases, results):
    c, w = cases[name], results[name].astype(np.float64)
    ok = c['d'] >= 1e-5
    err = np.abs(w - c['w'])
    print('%s: max |w - oracle| = %.3e over %d queries, %d left out; w in [%.3f, %.3f]'
          % (name, err[ok].max(), int(ok.sum()), int((~ok).sum()), w.min(), w.max()))
    assert np.isfinite(w).all()
    assert (~ok).sum() <= 0.001 * len(w)
    assert err[ok].max() <= TOL


# ---- 2 purity -----------------------------------------------------------------------------------------------------
def test_order_bins_batch_and_run_do_not_change_a_bit(cases, results):
    rng = np.random.default_rng(11)
    for name in ('open', 'soup'):
        m, P, want = cases[name]['mesh'], cases[name]['P'], results[name]
        perm = rng.permutation(len(P))
        assert same(run([m], [P[perm]])[0], want[perm]), (name, 'permutation')
        for bins in (1, 3, 8, 0):
            assert same(run([m], [P], bins=bins)[0], want), (name, bins)
        assert same(run([m], [P])[0], want), (name, 'alone, again')
    ms = [cases[n]['mesh'] for n in ('sphere', 'plate', 'soup', 'torus', 'open')]
    ps = [cases['sphere']['P'][:1000], np.zeros((0, 3)), cases['soup']['P'][:1], cases['torus']['P'],
          cases['open']['P'][:1]]
    got = run(ms, ps)
    assert same(got[0], results['sphere'][:1000]) and got[1].shape == (0,)
    assert same(got[2], results['soup'][:1]) and same(got[3], results['torus']) and same(got[4], results['open'][:1])


@pytest.mark.parametrize('n', [1, 63, 64, 65])
def test_query_counts_around_a_wave(n, cases, results):
    c = cases['torus']
    assert same(run([c['mesh']], [c['P'][3000:3000 + n]])[0], results['torus'][3000:3000 + n])


# ---- 3 signs and plumbing -----------------------------------------------------------------------------------------
def test_signs_and_plumbing(cases, results):
    from octfusion_amd import mesh_query as MQ
    ms = [to_dev(cases[n]['mesh']) for n in NAMES]
    ps = [pts_dev(cases[n]['P']) for n in NAMES]
    occ = MQ.occupancy(ms, ps)
    plain = MQ.closest_point(ms, ps, signed=False)
    parity = MQ.closest_point(ms, ps, signed=True)
    wind = MQ.closest_point(ms, ps, signed='winding')
    for k, name in enumerate(NAMES):
        inside = results[name] > 0.5
        assert occ[k].dtype == torch.bool and np.array_equal(occ[k].cpu().numpy(), inside)
        d0, d1, d2 = (x[k][0].cpu().numpy() for x in (plain, parity, wind))
        assert np.array_equal(np.abs(d2).view(np.int32), d0.view(np.int32))
        assert np.array_equal(np.signbit(d2), inside)
        assert torch.equal(wind[k][1], plain[k][1]) and torch.equal(wind[k][2], plain[k][2])
        differ = int((np.signbit(d1) != np.signbit(d2)).sum())
        print('%s: %d inside by winding number, %d signs differ from ray parity' % (name, int(inside.sum()), differ))
        if name in ('sphere', 'torus'):
            assert same(d2, d1)
        if name == 'open':
            assert differ > 0                                   # fails where any truthy `signed` still means parity
    with pytest.raises(ValueError, match="signed must be False, True or 'winding'"):
        MQ.closest_point(ms[:1], ps[:1], signed='parity')


def test_nested_and_overlapping_parts_add_up(cases):
    V, F = cases['soup']['mesh']
    g = np.linspace(-0.08, 0.08, 5)
    box = np.stack(np.meshgrid(g[g != 0] + 0.01, g, g, indexing='ij'), -1).reshape(-1, 3)     # off the plate's plane
    lens = np.array([[0.05, 0.0, 0.2], [0.05, 0.15, -0.15], [-0.02, -0.2, 0.1], [0.1, 0.05, -0.25]])  # both spheres
    P = np.concatenate([box, lens]).astype(np.float32).astype(np.float64)
    w = run([(V, F)], [P])[0].astype(np.float64)
    assert np.abs(w - W.exact(P, V, F)).max() <= TOL
    print('soup: w in the inner box %.3f .. %.3f, in the overlap %s' % (w[:len(box)].min(), w[:len(box)].max(),
                                                                         np.round(w[len(box):], 3)))
    assert (w >= 1.5).all()


# ---- 4 far field --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bins,beta', W.FAR_SETTINGS)
def test_far_field(bins, beta, cases, results):
    from octfusion_amd import _lib
    names = ['sphere', 'torus', 'open', 'soup']
    ms, ps = [cases[n]['mesh'] for n in names], [cases[n]['P'] for n in names]
    words = torch.zeros(4, dtype=torch.int64, device=dev())
    _lib.call('ofx_mesh_winding_set_counters', _lib.ptr(words))
    try:
        got = run(ms, ps, bins=bins, beta=beta)
        torch.cuda.synchronize()
    finally:
        _lib.call('ofx_mesh_winding_set_counters', None)
    far_bins, staged, pairs, dipoles = (int(x) for x in words.cpu())
    brute = sum(len(cases[n]['P']) * len(cases[n]['mesh'][1]) for n in names)
    print('bins %d beta %g: %d wave-far bins, %d dipoles, %d pairs = %.1f %% of brute force'
          % (bins, beta, far_bins, dipoles, pairs, 100.0 * pairs / brute))
    assert dipoles > 0 and far_bins > 0 and 0 < pairs < brute
    for name, w in zip(names, got):
        c = cases[name]
        wf, margin, E = far_oracle(cases, name, bins, beta)
        w64 = w.astype(np.float64)
        proof = margin > 1e-9
        ea = np.abs(w64 - wf)[proof].max()
        eb = np.abs(w64 - c['w']).max()
        clear = np.abs(c['w'] - 0.5) > 2 * E
        flips = int(((w64 > 0.5) != (c['w'] > 0.5))[clear].sum())
        print('  %s: E = %.3e; (a) %.3e on %d margin-proof queries; (b) %.3e; (c) %d flips, %d left out'
              % (name, E, ea, int(proof.sum()), eb, flips, int((~clear).sum())))
        assert (~proof).sum() <= 0.001 * len(w) and ea <= TOL
        assert eb <= 2 * E + TOL
        assert (~clear).sum() <= 0.01 * len(w) and flips == 0
    # the same bits from a second run, under a permutation and alone
    again = run(ms, ps, bins=bins, beta=beta)
    assert all(same(a, b) for a, b in zip(again, got))
    perm = np.random.default_rng(5).permutation(W.N_QUERIES)
    assert same(run([ms[3]], [ps[3][perm]], bins=bins, beta=beta)[0], got[3][perm])
    assert same(run([ms[2]], [ps[2][:777]], bins=bins, beta=beta)[0], got[2][:777])


# ---- 5 frames and corner cases ------------------------------------------------------------------------------------
def test_a_mesh_in_another_frame(cases):
    c = cases['open']
    V, F = c['mesh']
    shift = np.array([100.0, -50.0, 7.0])
    V2 = (V * 40 + shift).astype(np.float32).astype(np.float64)
    P2 = (c['P'] * 40 + shift).astype(np.float32).astype(np.float64)
    ok = Q.query(P2, V2, F)[0] >= 40 * 1e-5
    w = run([(V2, F)], [P2])[0].astype(np.float64)
    err = np.abs(w - W.exact(P2, V2, F))
    print('moved open sphere: exact %.3e over %d queries' % (err[ok].max(), int(ok.sum())))
    assert (~ok).sum() <= 0.001 * len(w) and err[ok].max() <= TOL
    wf, margin, _ = W.far(P2, V2, F, 4, 2.0)
    got = run([(V2, F)], [P2], bins=4, beta=2.0)[0].astype(np.float64)
    proof = margin > 1e-9
    print('moved open sphere: far field %.3e over %d margin-proof queries' % (np.abs(got - wf)[proof].max(),
                                                                              int(proof.sum())))
    assert (~proof).sum() <= 0.001 * len(w) and np.abs(got - wf)[proof].max() <= TOL


def test_non_finite_queries(cases, results):
    c = cases['sphere']
    P = c['P'][:300].copy()
    bad = [0, 7, 63, 64, 100, 299]
    P[0] = [np.nan, 0, 0]
    P[7] = [0, np.inf, 0]
    P[63] = [0, 0, -np.inf]
    P[64] = [np.nan, np.nan, np.nan]
    P[100] = [np.inf, np.nan, 0.1]
    P[299] = [0.2, np.nan, 0.1]
    good = np.setdiff1d(np.arange(300), bad)
    w = run([c['mesh']], [P])[0]
    assert np.isnan(w[bad]).all() and same(w[good], results['sphere'][good])
    ref = run([c['mesh']], [c['P'][:300]], bins=4, beta=2.0)[0]
    w = run([c['mesh']], [P], bins=4, beta=2.0)[0]
    assert np.isnan(w[bad]).all() and same(w[good], ref[good])
    assert np.isnan(run([c['mesh']], [np.full((70, 3), np.nan)])[0]).all()
    from octfusion_amd import mesh_query as MQ
    assert not MQ.occupancy([to_dev(c['mesh'])], [pts_dev(P)])[0].cpu().numpy()[bad].any()


def test_queries_on_the_surface_are_finite(cases):
    V, F = cases['plate']['mesh']
    P = np.array([V[0], V[2], [V[0, 0], 0.9, 0.2], [V[0, 0], -0.7, -0.9], [V[0, 0], 0.1, 0.2]])
    with np.errstate(all='ignore'):
        want = W.exact(P, V, F)
    w = run([(V, F)], [P])[0].astype(np.float64)
    print('plate: on two vertices, in the plane outside, in a face: device %s oracle %s' % (w, want))
    assert np.isfinite(w).all() and np.isfinite(want).all()
    assert np.abs(w - want).max() <= TOL
    assert (w[2:4] == 0).all() and abs(abs(w[4]) - 0.5) <= TOL


def test_zero_area_and_doubled_faces(cases, results):
    c = cases['sphere']
    V, F = c['mesh']
    flat = np.array([[5, 5, 5], [3, 9, 3], [0, 1, 1]], np.int32)
    mixed = (V, np.concatenate([flat[:1], F[:700], flat[1:], F[700:]]))
    assert same(run([mixed], [c['P']])[0], results['sphere'])            # skipped terms leave the chain as it is
    only = (V, flat)
    assert (run([only], [c['P'][:200]])[0] == 0).all()
    assert (run([only], [c['P'][:200]], bins=2, beta=2.0)[0] == 0).all()
    twice = (V, np.concatenate([F, F]))
    w = run([twice], [c['P']])[0].astype(np.float64)
    ok = c['d'] >= 1e-5
    assert np.abs(w - 2 * c['w'])[ok].max() <= TOL
    inside = c['w'] > 0.5
    assert np.abs(w[inside & ok] - 2).max() <= 1e-5 and np.abs(w[~inside & ok]).max() <= 1e-5


def raw_winding(meshes, sets, bins=0, beta=0.0):
    """ofx_mesh_winding itself: (return code, status, w) with the outputs prefilled with a sentinel."""
    from octfusion_amd import _lib
    vs = torch.cat([to_dev(m)[0] for m in meshes])
    fs = torch.cat([to_dev(m)[1] for m in meshes])
    q = torch.cat([pts_dev(P) for P in sets])
    nv, nf, nq = [len(m[0]) for m in meshes], [len(m[1]) for m in meshes], [len(P) for P in sets]
    offs = torch.from_numpy(np.stack([np.cumsum([0] + nv), np.cumsum([0] + nf), np.cumsum([0] + nq)])).to(dev())
    B, Qn = len(meshes), sum(nq)
    nbytes = _lib.lib().ofx_mesh_winding_ws_bytes(B, sum(nv), sum(nf), Qn, bins if 0 <= bins <= 16 else 0)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev())
    w = torch.full((Qn,), 77.0, device=dev())
    status = torch.full((B,), 77, dtype=torch.int32, device=dev())
    rc = _lib.lib().ofx_mesh_winding(vs.data_ptr(), fs.data_ptr(), offs[0].data_ptr(), offs[1].data_ptr(),
                                     q.data_ptr(), offs[2].data_ptr(), B, Qn, max(nq), bins, beta, w.data_ptr(),
                                     ws.data_ptr(), status.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    return rc, status.cpu().numpy(), np.split(w.cpu().numpy(), np.cumsum(nq)[:-1])


def test_a_bad_shape_is_refused_alone(cases, results):
    from octfusion_amd import mesh_query as MQ
    s, t = cases['sphere'], cases['torus']
    V, F = t['mesh']
    bad_index = (V, F.copy())
    bad_index[1][17, 1] = len(V)
    nan_vertex = (V.copy(), F)
    nan_vertex[0][F[40, 2], 0] = np.nan
    for bad in (bad_index, nan_vertex):
        for kw in ({}, {'bins': 4, 'beta': 2.0}):
            rc, status, w = raw_winding([s['mesh'], bad, s['mesh']], [s['P'][:200], t['P'][:100], s['P'][:50]], **kw)
            assert rc == 0 and status.tolist() == [0, 1, 0]
            assert (w[1] == 77).all()                               # left unwritten
            if not kw:
                assert same(w[0], results['sphere'][:200]) and same(w[2], results['sphere'][:50])
        for fn in (MQ.winding_number, MQ.occupancy):
            with pytest.raises(ValueError, match='shape 1 has a face index outside'):
                fn([to_dev(s['mesh']), to_dev(bad), to_dev(s['mesh'])],
                   [pts_dev(s['P'][:8]), pts_dev(t['P'][:8]), pts_dev(s['P'][:8])])


def test_wrong_arguments_raise_before_a_launch(cases):
    from octfusion_amd import _lib, mesh_query as MQ
    m = to_dev(cases['plate']['mesh'])
    p = pts_dev(cases['plate']['P'][:10])
    for fn in (MQ.winding_number, MQ.occupancy):
        for bins in (-1, 17):
            with pytest.raises(ValueError, match='bins'):
                fn([m], [p], bins=bins)
        for beta in (-1.0, float('nan'), float('inf')):
            with pytest.raises(ValueError, match='beta'):
                fn([m], [p], beta=beta)
        with pytest.raises(ValueError, match='float32'):
            fn([m], [p.double()])
        with pytest.raises(ValueError, match='float32 vertices and int32 faces'):
            fn([(m[0], m[1].long())], [p])
        with pytest.raises(ValueError, match=r'\[n, 3\]'):
            fn([m], [p[:, :2]])
        with pytest.raises(ValueError, match=r'\[B, n, 3\]'):
            fn([m], p)
        with pytest.raises(ValueError, match='2 point sets for 1 meshes'):
            fn([m], [p, p])
        with pytest.raises(ValueError, match='not on the device'):
            fn([m], [p.cpu()])
        with pytest.raises(ValueError, match='shape 0 has no faces'):
            fn([(m[0], m[1][:0])], [p])
        with pytest.raises(ValueError, match='no meshes'):
            fn([], [])
    stacked = MQ.winding_number([m, m], torch.stack([p, p]))
    assert torch.equal(stacked[0], stacked[1]) and stacked[0].shape == (10,)
    L = _lib.lib()
    assert L.ofx_mesh_winding_ws_bytes(1, 8, 12, 10, 17) == 0 and L.ofx_mesh_winding_ws_bytes(0, 8, 12, 10, 0) == 0
    assert L.ofx_mesh_winding_ws_bytes(1, 8, 12, -1, 0) == 0 and L.ofx_mesh_winding_ws_bytes(1, 8, 0, 10, 0) == 0
    plate = cases['plate']
    for kw in ({'bins': 17}, {'bins': -1}, {'beta': -1.0}, {'beta': float('nan')}, {'beta': float('inf')}):
        rc, status, w = raw_winding([plate['mesh']], [plate['P'][:10]], **kw)
        assert rc == -1 and status.tolist() == [77] and (w[0] == 77).all(), kw


# ---- 6 lattice ----------------------------------------------------------------------------------------------------
def test_lattice(cases):
    from octfusion_amd import mesh2sdf as M
    sphere, opened = to_dev(cases['sphere']['mesh']), to_dev(cases['open']['mesh'])
    S = 16
    lat = M.mesh_to_sdf([sphere, opened], S, signed='winding')
    parity = M.mesh_to_sdf([sphere, opened], S, signed=True)
    plain = M.mesh_to_sdf([sphere, opened], S, signed=False)
    assert lat.shape == (2, S, S, S) and lat.dtype == torch.float32
    assert torch.equal(lat[0].view(torch.int32), parity[0].view(torch.int32))
    assert torch.equal(lat.abs().view(torch.int32), plain.view(torch.int32))
    assert torch.equal(M.mesh_to_sdf([opened], S, signed='winding')[0].view(torch.int32), lat[1].view(torch.int32))
    P = O.lattice(S)
    V, F = cases['open']['mesh']
    w, d = W.exact(P, V, F), O.udf(P, V, F)
    ok = (d >= 1e-5) & (np.abs(w - 0.5) > TOL)
    got = lat[1].cpu().numpy().reshape(-1)
    print('open sphere, S = %d: %d of %d lattice points inside by winding number, %d by parity, %d left out'
          % (S, int((got < 0).sum()), len(got), int((parity[1] < 0).sum()), int((~ok).sum())))
    assert np.array_equal((got < 0)[ok], (w > 0.5)[ok]) and ok.sum() >= 0.999 * len(ok)
    assert not torch.equal(lat[1], parity[1])
    # compute() on the same mesh: the same lattice
    one = M.compute(V, F, S, fix=False, sign='winding')
    assert torch.equal(one.view(torch.int32), lat[1].view(torch.int32))
    assert torch.equal(M.compute(V, F, S, fix=False).view(torch.int32), parity[1].view(torch.int32))
    with pytest.raises(ValueError, match='sign'):
        M.compute(V, F, S, fix=False, sign='rays')
    with pytest.raises(ValueError, match='signed must be'):
        M.mesh_to_sdf([opened], S, signed='rays')
    fast = M.mesh_to_sdf([opened], S, signed='winding', beta=3.0)
    assert torch.equal(fast.abs().view(torch.int32), plain[1:].view(torch.int32))
    assert ((fast[0] < 0) != (lat[1] < 0)).sum() <= 0.01 * S ** 3


def test_command_lines(tmp_path, cases):
    from octfusion_amd import mesh, mesh2sdf as M
    V, F = cases['open']['mesh']
    a, b = str(tmp_path / 'a.obj'), str(tmp_path / 'open.obj')
    mesh.write_obj(a, *O.icosphere(2, (0.07, -0.05, -0.1), 0.2))          # well inside the open sphere, off its hole
    mesh.write_obj(b, V, F)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, '-m', 'octfusion_amd.mesh_query', '--a', a, '--b', b, '--samples', '2000',
                          '--signed', 'winding'], capture_output=True, text=True, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    e = json.loads(out.stdout.strip().splitlines()[-1])
    print('mesh_query --signed winding:', e)
    assert e['samples'] == 2000
    assert e['a_to_b']['mean'] < -0.1 and abs(e['a_to_b']['mean']) <= e['a_to_b']['rms'] <= e['a_to_b']['max']
    assert e['b_to_a']['mean'] > 0.1                                      # b's samples lie outside a
    root = str(tmp_path / 'data')
    out = subprocess.run([sys.executable, '-m', 'octfusion_amd.mesh2sdf', '--input', b, '--out', root, '--size', '16',
                          '--sign', 'winding'], capture_output=True, text=True, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    sdf = np.load(os.path.join(root, 'sdf', 'open.npy'))
    rv, rf = M.read_mesh(b)
    from octfusion_amd import mesh_query as MQ
    assert MQ.DEFAULT_CLI_BETA == M.parser().get_default('beta') == MQ.parser().get_default('beta') > 0
    want = M.compute(M.normalize(rv)[0], rf, 16, fix=False, sign='winding', beta=MQ.DEFAULT_CLI_BETA).cpu().numpy()
    assert sdf.shape == (16, 16, 16) and np.array_equal(sdf.view(np.int32), want.view(np.int32))
    assert 0 < (sdf < 0).sum() < sdf.size // 2
    assert all(os.path.exists(os.path.join(root, *p)) for p in (('mesh', 'open.obj'), ('bbox', 'open.npz')))
