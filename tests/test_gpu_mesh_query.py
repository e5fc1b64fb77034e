"""GPU tests of the point -> mesh queries (csrc/ofx_meshquery.hip, octfusion_amd/mesh_query.py) against the float64
oracle (tests/meshquery_oracle.py: brute force with Ericson's regions; winding-number sign).

Shapes and query sets: meshquery_oracle.shapes() / query_sets() -- icosphere(2) 320 faces, torus(16, 8) 256, box 12,
plate 2; per shape 3072 points uniform in [-1.2, 1.2]^3 plus 1024 vertices jittered by N(0, 0.02), default_rng(7),
fp32.  tests/test_meshquery_oracle.py establishes on the CPU that no query lies within 1e-5 of its mesh and that 578,
464 and 346 queries fall inside the closed shapes.

Tolerances.
  values  |got - oracle| <= 1e-5 + 1e-5 |oracle|, the bound and derivation of test_gpu_mesh2sdf.py: coordinates are
          <= 2 in magnitude, the kernel evaluates in fp64 and rounds once (<= 2^-24 |value|).  In the moved frame
          (x 40, + (100, -50, 7)) the same bound times 40: the moved vertices and queries are rounded to fp32 at
          magnitude <= 150, half an ulp of 7.6e-6 per coordinate, 1.3e-5 per point pair, far inside 4e-4.
  signs   equal to the oracle's wherever the oracle distance is >= 1e-5; at most 0.1 % left out (here: none).
  faces   never compared by index with the oracle (ties between faces are the normal case outside a convex mesh):
          the oracle distance to the RETURNED face alone is within the value bound of the minimum, the returned point
          is within 1e-5 of that face, and | |q - point| - dist | <= 1e-5 (fp32 rounding of three coordinates
          <= 1.3: 3 * 2^-24 * 1.3 = 2.3e-7, and of dist).
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

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOSED = ['sphere', 'torus', 'box']
ALL = CLOSED + ['plate']


def dev():
    return torch.device('cuda:0')


def to_dev(m):
    v, f = m
    return (torch.from_numpy(np.asarray(v, np.float32)).to(dev()), torch.from_numpy(np.asarray(f, np.int32)).to(dev()))


def pts_dev(P):
    return torch.from_numpy(np.ascontiguousarray(P, np.float32)).to(dev())


def run(meshes, sets, **kw):
    """closest_point on numpy meshes and query sets -> per mesh (dist fp32, face int32, point fp32 or None), numpy."""
    from octfusion_amd import mesh_query as MQ
    out = MQ.closest_point([to_dev(m) for m in meshes], [pts_dev(P) for P in sets], **kw)
    assert len(out) == len(meshes)
    res = []
    for (d, f, p), P in zip(out, sets):
        assert d.shape == (len(P),) and d.dtype == torch.float32 and f.shape == (len(P),) and f.dtype == torch.int32
        assert (p is None) == (kw.get('want_point', True) is False)
        assert p is None or (p.shape == (len(P), 3) and p.dtype == torch.float32)
        res.append((d.cpu().numpy(), f.cpu().numpy(), None if p is None else p.cpu().numpy()))
    return res


def same(a, b):
    """Bitwise equality of two result triples (NaNs included)."""
    return all((x is None and y is None) or np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def check_values(got, ref, what, scale=1.0):
    got = got.astype(np.float64)
    err = np.abs(got - ref)
    worst = (err - 1e-5 * np.abs(ref)).max()
    print('%s: max |got - oracle| = %.3e over %d queries' % (what, err.max(), len(ref)))
    assert np.isfinite(got).all()
    assert worst <= 1e-5 * scale


@pytest.fixture(scope='module')
def cases():
    meshes = Q.shapes()
    sets = Q.query_sets([m for _, m in meshes])
    out = {}
    for (name, m), P in zip(meshes, sets):
        d, face, point = Q.query(P, *m)
        out[name] = {'mesh': m, 'P': P, 'd': d, 'face': face, 'point': point,
                     'inside': Q.inside(P, *m) if name in CLOSED else None}
    return out


@pytest.fixture(scope='module')
def results(cases):
    """The device results of the four shapes, unsigned and signed, one call each (shared by tests 1 - 3)."""
    ms, ps = [cases[n]['mesh'] for n in ALL], [cases[n]['P'] for n in ALL]
    return {'unsigned': dict(zip(ALL, run(ms, ps))), 'signed': dict(zip(ALL, run(ms, ps, signed=True)))}


# ---- 1 values -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ALL)
def test_values(name, cases, results):
    c = cases[name]
    u, s = results['unsigned'][name][0], results['signed'][name][0]
    assert (u >= 0).all()
    check_values(u, c['d'], name + ' unsigned')
    check_values(np.abs(s), c['d'], name + ' signed')
    assert np.array_equal(np.abs(s).view(np.int32), u.view(np.int32))


# ---- 2 signs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CLOSED)
def test_signs(name, cases, results):
    c = cases[name]
    s = results['signed'][name][0]
    ok = c['d'] >= 1e-5
    left_out = int((~ok).sum())
    wrong = int(((s < 0) != c['inside'])[ok].sum())
    print('%s: %d of %d queries left out of the sign check, %d wrong, %d inside' % (name, left_out, len(s), wrong,
                                                                                   int(c['inside'].sum())))
    assert left_out <= 0.001 * len(s) and left_out == 0
    assert wrong == 0
    assert int((s < 0).sum()) == {'sphere': 578, 'torus': 464, 'box': 346}[name]


def test_open_mesh_gives_the_parity(cases, results):
    """What a caller sees on an open mesh: negative exactly behind the plate (x = fp32(0.03), |y|, |z| < 0.5) as seen
    from -x.  The plate's plane has constant x, so x_cross is that x exactly and the rule x_cross <= q.x is decided
    without rounding; no query of the set lies exactly on a plane through the plate's rim."""
    P, s = cases['plate']['P'], results['signed']['plate'][0]
    x0 = float(cases['plate']['mesh'][0][0, 0])
    assert x0 == float(np.float32(0.03)) and (np.abs(P[:, 1:]) != 0.5).all()
    behind = (P[:, 0] >= x0) & (np.abs(P[:, 1]) < 0.5) & (np.abs(P[:, 2]) < 0.5)
    assert 100 < behind.sum() < len(P) - 100
    assert np.array_equal(s < 0, behind)


# ---- 3 face and point, tie-proof ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ALL)
def test_face_and_point(name, cases, results):
    c = cases[name]
    V, F = c['mesh']
    for kind in ('unsigned', 'signed'):
        dist, face, point = results[kind][name]
        assert face.min() >= 0 and face.max() < len(F)
        d_face, _ = Q.to_face(c['P'], V, F, face)
        over = d_face - c['d']
        print('%s %s: the returned face is at most %.3e farther than the nearest; %d of %d indices differ from the '
              "oracle's" % (name, kind, over.max(), int((face != c['face']).sum()), len(face)))
        assert (over <= 1e-5 + 1e-5 * c['d']).all()
        off_face, _ = Q.to_face(point.astype(np.float64), V, F, face)
        assert off_face.max() <= 1e-5
        gap = np.abs(np.linalg.norm(c['P'] - point.astype(np.float64), axis=1) - np.abs(dist.astype(np.float64)))
        assert gap.max() <= 1e-5
    assert same(results['unsigned'][name][1:], results['signed'][name][1:])


# ---- 4 tie rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['sphere', 'box', 'plate'])
def test_doubled_faces_return_the_lower_index(name, cases, results):
    V, F = cases[name]['mesh']
    twice = (V, np.concatenate([F, F]))
    for signed in (False, True):
        got = run([twice], [cases[name]['P']], signed=signed)[0]
        assert got[1].max() < len(F)
        # the doubled mesh crosses every ray twice: its parity is even everywhere, the magnitude is unchanged
        want = results['signed' if signed else 'unsigned'][name]
        if signed:
            assert (got[0] >= 0).all() and np.array_equal(got[0].view(np.int32), np.abs(want[0]).view(np.int32))
            assert same(got[1:], want[1:])
        else:
            assert same(got, want)


# ---- 5 the lattice identity ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CLOSED)
def test_lattice_points_give_the_lattice_bits(name, cases):
    from octfusion_amd import mesh2sdf as M
    m = cases[name]['mesh']
    if name == 'box':
        assert np.array_equal(m[0], O.box(-0.5, 0.5)[0])          # lattice aligned: rays through diagonals and vertices
    P = O.lattice(16)
    assert np.array_equal(P.astype(np.float32).astype(np.float64), P)
    for signed in (False, True):
        lat = M.mesh_to_sdf([to_dev(m)], 16, signed).cpu().numpy().reshape(-1)
        got = run([m], [P], signed=signed, want_point=False)[0][0]
        diff = int((lat.view(np.int32) != got.view(np.int32)).sum())
        print('%s signed=%s: %d of %d lattice values differ in a bit; %d negative' % (name, signed, diff, len(lat),
                                                                                      int((lat < 0).sum())))
        assert diff == 0


# ---- 6 purity -----------------------------------------------------------------------------------------------------
def test_order_bins_and_batch_do_not_change_a_bit(cases, results):
    rng = np.random.default_rng(11)
    for name in ('torus', 'box'):
        m, P = cases[name]['mesh'], cases[name]['P']
        for signed in (False, True):
            want = results['signed' if signed else 'unsigned'][name]
            perm = rng.permutation(len(P))
            got = run([m], [P[perm]], signed=signed)[0]
            assert same(got, tuple(x[perm] for x in want)), (name, 'permutation')
            for bins in (1, 3, 16, 0):
                assert same(run([m], [P], signed=signed, bins=bins)[0], want), (name, bins)
    # alone against a batch of three shapes with different query counts, one of them zero
    ms = [cases['sphere']['mesh'], cases['plate']['mesh'], cases['torus']['mesh']]
    ps = [cases['sphere']['P'][:1000], np.zeros((0, 3)), cases['torus']['P'][:777]]
    for signed in (False, True):
        key = 'signed' if signed else 'unsigned'
        got = run(ms, ps, signed=signed)
        assert same(got[0], tuple(x[:1000] for x in results[key]['sphere']))
        assert got[1][0].shape == (0,) and got[1][2].shape == (0, 3)
        assert same(got[2], tuple(x[:777] for x in results[key]['torus']))


# ---- 7 frames -----------------------------------------------------------------------------------------------------
def test_a_mesh_in_another_frame(cases, results):
    c = cases['torus']
    V, F = c['mesh']
    shift = np.array([100.0, -50.0, 7.0])
    V2 = (V * 40 + shift).astype(np.float32).astype(np.float64)
    P2 = (c['P'] * 40 + shift).astype(np.float32).astype(np.float64)
    want = results['signed']['torus']
    dist, face, point = run([(V2, F)], [P2], signed=True)[0]
    check_values(dist, 40 * want[0].astype(np.float64), 'moved torus against 40 x the unmoved device result', scale=40)
    check_values(np.abs(dist), 40 * c['d'], 'moved torus against 40 x the oracle', scale=40)
    assert np.array_equal(dist < 0, want[0] < 0)
    every = np.sort(Q.all_faces(c['P'], V, F), axis=1)
    clear = every[:, 1] - every[:, 0] > 1e-4                    # the runner-up face is clearly farther
    print('moved torus: %d of %d queries have a clear nearest face' % (clear.sum(), len(clear)))
    assert clear.sum() > len(clear) // 8                        # (two faces tie along every edge and vertex region)
    assert np.array_equal(face[clear], want[1][clear]) and np.array_equal(face[clear], c['face'][clear])


# ---- 8 geometry of a wave -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 63, 64, 65])
def test_query_counts_around_a_wave(n, cases, results):
    c = cases['sphere']
    for signed in (False, True):
        got = run([c['mesh']], [c['P'][3000:3000 + n]], signed=signed)[0]
        assert same(got, tuple(x[3000:3000 + n] for x in results['signed' if signed else 'unsigned']['sphere']))


def test_clusters_far_apart_and_identical_queries(cases, results):
    c = cases['torus']
    V, F = c['mesh']
    rng = np.random.default_rng(3)
    # two clusters 2.4 apart in one wave (32 queries each): a box over both spans the whole mesh
    a = np.array([-1.2, 0.1, 0.0]) + rng.normal(0, 0.01, (32, 3))
    b = np.array([1.2, 0.1, 0.0]) + rng.normal(0, 0.01, (32, 3))
    P = np.concatenate([a, b]).astype(np.float32).astype(np.float64)
    d, _, _ = Q.query(P, V, F)
    got = run([c['mesh']], [P], signed=True)[0]
    check_values(got[0], d, 'two clusters')                     # all outside: positive
    d_face, _ = Q.to_face(P, V, F, got[1])
    assert (d_face - d <= 1e-5 + 1e-5 * d).all()
    # three clusters in one wave: cutting the wave at its longest step still leaves a part that spans two of them
    third = np.array([0.0, -1.2, 0.9]) + rng.normal(0, 0.01, (20, 3))
    P = np.concatenate([a[:22], b[:22], third]).astype(np.float32).astype(np.float64)
    d, _, _ = Q.query(P, V, F)
    got = run([c['mesh']], [P], signed=True)[0]
    check_values(got[0], d, 'three clusters')
    d_face, _ = Q.to_face(P, V, F, got[1])
    assert (d_face - d <= 1e-5 + 1e-5 * d).all()
    # all queries identical: the wave's box is a point; every lane returns the same bits, those of a single query
    one = c['P'][5:6]
    many = run([c['mesh']], [np.repeat(one, 200, axis=0)], signed=True)[0]
    single = tuple(x[5:6] for x in results['signed']['torus'])
    assert same(many, tuple(np.repeat(x, 200, axis=0) for x in single))


def test_many_bins_and_staging_rounds():
    m = O.icosphere(4, (0.07, -0.05, 0.03), 0.55)
    assert len(m[1]) == 5120                                    # automatic bins: 5^3; bins = 1: 80 staging rounds
    P = Q.query_sets([m], seed=5, n_uniform=384, n_near=128)[0]
    d, _, _ = Q.query(P, *m)
    inside = Q.inside(P, *m)
    assert d.min() >= 1e-5
    got = run([m], [P], signed=True)[0]
    check_values(np.abs(got[0]), d, 'icosphere(4)')
    assert np.array_equal(got[0] < 0, inside)
    d_face, _ = Q.to_face(P, *m, got[1])
    assert (d_face - d <= 1e-5 + 1e-5 * d).all()
    for bins in (1, 2, 16):
        assert same(run([m], [P], signed=True, bins=bins)[0], got), bins


# ---- 9 bad input --------------------------------------------------------------------------------------------------
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
    for signed in (False, True):
        dist, face, point = run([c['mesh']], [P], signed=signed)[0]
        assert np.isnan(dist[bad]).all() and (face[bad] == -1).all() and np.isnan(point[bad]).all()
        want = results['signed' if signed else 'unsigned']['sphere']
        assert same((dist[good], face[good], point[good]), tuple(x[good] for x in want))
    # a set of nothing but non-finite queries
    dist, face, point = run([c['mesh']], [np.full((70, 3), np.nan)])[0]
    assert np.isnan(dist).all() and (face == -1).all() and np.isnan(point).all()


def raw_query(meshes, sets, bins=0, signed=0):
    """ofx_mesh_query itself: (return code, status, dist, face, point) with the outputs prefilled with a sentinel."""
    from octfusion_amd import _lib
    vs = torch.cat([to_dev(m)[0] for m in meshes])
    fs = torch.cat([to_dev(m)[1] for m in meshes])
    q = torch.cat([pts_dev(P) for P in sets])
    nv, nf, nq = [len(m[0]) for m in meshes], [len(m[1]) for m in meshes], [len(P) for P in sets]
    offs = torch.from_numpy(np.stack([np.cumsum([0] + nv), np.cumsum([0] + nf), np.cumsum([0] + nq)])).to(dev())
    B, Qn = len(meshes), sum(nq)
    nbytes = _lib.lib().ofx_mesh_query_ws_bytes(B, sum(nv), sum(nf), Qn, max(bins, 0) if bins <= 16 else 0)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev())
    dist = torch.full((Qn,), 77.0, device=dev())
    face = torch.full((Qn,), 77, dtype=torch.int32, device=dev())
    point = torch.full((Qn, 3), 77.0, device=dev())
    status = torch.full((B,), 77, dtype=torch.int32, device=dev())
    rc = _lib.lib().ofx_mesh_query(vs.data_ptr(), fs.data_ptr(), offs[0].data_ptr(), offs[1].data_ptr(), q.data_ptr(),
                                   offs[2].data_ptr(), B, Qn, max(nq), bins, signed, dist.data_ptr(), face.data_ptr(),
                                   point.data_ptr(), ws.data_ptr(), status.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    cuts = np.cumsum(nq)[:-1]
    return (rc, status.cpu().numpy(), np.split(dist.cpu().numpy(), cuts), np.split(face.cpu().numpy(), cuts),
            np.split(point.cpu().numpy(), cuts))


def test_a_bad_shape_is_refused_alone(cases, results):
    from octfusion_amd import mesh_query as MQ
    s, t = cases['sphere'], cases['torus']
    V, F = t['mesh']
    bad_index = (V, F.copy())
    bad_index[1][17, 1] = len(V)
    nan_vertex = (V.copy(), F)
    nan_vertex[0][F[40, 2], 0] = np.nan
    unused_nan = (np.concatenate([V, [[np.nan] * 3]]), F)        # a vertex no face uses may be anything
    for bad in (bad_index, nan_vertex):
        rc, status, dist, face, point = raw_query([s['mesh'], bad, s['mesh']],
                                                  [s['P'][:200], t['P'][:100], s['P'][:50]], signed=1)
        assert rc == 0 and status.tolist() == [0, 1, 0]
        assert (dist[1] == 77).all() and (face[1] == 77).all() and (point[1] == 77).all()     # left unwritten
        want = results['signed']['sphere']
        assert same((dist[0], face[0], point[0]), tuple(x[:200] for x in want))
        assert same((dist[2], face[2], point[2]), tuple(x[:50] for x in want))
        with pytest.raises(ValueError, match='shape 1 has a face index outside'):
            MQ.closest_point([to_dev(s['mesh']), to_dev(bad), to_dev(s['mesh'])],
                             [pts_dev(s['P'][:8]), pts_dev(t['P'][:8]), pts_dev(s['P'][:8])])
    got = run([unused_nan], [t['P'][:500]], signed=True)[0]
    assert same(got, tuple(x[:500] for x in results['signed']['torus']))


def test_zero_area_triangles(cases, results):
    """Degenerate faces are the segment or point they are: appended to the torus they change nothing where they are
    farther than the surface, and alone they give segment and point distances."""
    V = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.5, 0.5, 0.5]])
    F = np.array([[0, 1, 2], [3, 3, 3], [0, 2, 2]], np.int32)
    P = np.concatenate([np.array([[1.5, 1.0, 0.0], [3.0, 0.0, 4.0], [0.5, 0.5, 0.75]]),
                        np.random.default_rng(2).uniform(-1, 3, (200, 3))]).astype(np.float32).astype(np.float64)
    d, _, _ = Q.query(P, V, F)
    for signed in (False, True):                                 # no projected area: nothing is ever crossed
        dist, face, point = run([(V, F)], [P], signed=signed)[0]
        check_values(dist, d, 'degenerate faces')
        d_face, _ = Q.to_face(P, V, F, face)
        assert (d_face - d <= 1e-5 + 1e-5 * d).all()
        assert np.abs(np.linalg.norm(P - point, axis=1) - dist).max() <= 1e-5
    assert face[:3].tolist() == [0, 0, 1]
    t = cases['torus']
    TV, TF = t['mesh']
    far = (np.concatenate([TV, [[5.0, 5.0, 5.0], [6.0, 5.0, 5.0]]]),
           np.concatenate([TF, [[len(TV), len(TV), len(TV)], [len(TV), len(TV) + 1, len(TV)]]]).astype(np.int32))
    assert same(run([far], [t['P']], signed=True)[0], results['signed']['torus'])


def test_wrong_arguments_raise_before_a_launch(cases):
    from octfusion_amd import _lib, mesh_query as MQ
    m = to_dev(cases['box']['mesh'])
    p = pts_dev(cases['box']['P'][:10])
    for bins in (-1, 17):
        with pytest.raises(ValueError, match='bins'):
            MQ.closest_point([m], [p], bins=bins)
    with pytest.raises(ValueError, match='float32'):
        MQ.closest_point([m], [p.double()])
    with pytest.raises(ValueError, match='float32 vertices and int32 faces'):
        MQ.closest_point([(m[0], m[1].long())], [p])
    with pytest.raises(ValueError, match=r'\[n, 3\]'):
        MQ.closest_point([m], [p[:, :2]])
    with pytest.raises(ValueError, match=r'\[B, n, 3\]'):
        MQ.closest_point([m], p)
    with pytest.raises(ValueError, match='2 point sets for 1 meshes'):
        MQ.closest_point([m], [p, p])
    with pytest.raises(ValueError, match='not on the device'):
        MQ.closest_point([m], [p.cpu()])
    with pytest.raises(ValueError, match='shape 0 has no faces'):
        MQ.closest_point([(m[0], m[1][:0])], [p])
    with pytest.raises(ValueError, match='no meshes'):
        MQ.closest_point([], [])
    stacked = MQ.closest_point([m, m], torch.stack([p, p]))
    assert torch.equal(stacked[0][0], stacked[1][0]) and stacked[0][2].shape == (10, 3)
    # the C entry refuses what the wrapper would not pass on
    L = _lib.lib()
    assert L.ofx_mesh_query_ws_bytes(1, 8, 12, 10, 17) == 0 and L.ofx_mesh_query_ws_bytes(0, 8, 12, 10, 0) == 0
    assert L.ofx_mesh_query_ws_bytes(1, 8, 12, -1, 0) == 0 and L.ofx_mesh_query_ws_bytes(1, 8, 0, 10, 0) == 0
    small, big = L.ofx_mesh_query_ws_bytes(1, 8, 12, 10, 4), L.ofx_mesh_query_ws_bytes(1, 8, 1012, 10, 4)
    assert big - small >= 1000 * 40 - 256 and big - small <= 1000 * 40 + 256      # 36 + 4 bytes per face
    box = cases['box']
    rc, status, dist, face, point = raw_query([box['mesh']], [box['P'][:10]], bins=17)
    assert rc == -1 and status.tolist() == [77] and (dist[0] == 77).all()
    rc, status, dist, face, point = raw_query([box['mesh']], [box['P'][:10]], bins=-1)
    assert rc == -1 and status.tolist() == [77] and (dist[0] == 77).all()


# ---- 10 uses ------------------------------------------------------------------------------------------------------
def test_mesh_error(cases):
    from octfusion_amd import mesh_query as MQ
    m = cases['torus']['mesh']
    e = MQ.mesh_error(m, m, n=4000, seed=1)
    print('mesh_error(m, m):', e)
    assert set(e) == {'a_to_b', 'b_to_a', 'hausdorff', 'samples'} and set(e['a_to_b']) == {'mean', 'rms', 'max'}
    assert e['hausdorff'] == max(e['a_to_b']['max'], e['b_to_a']['max']) <= 1e-6
    # concentric icospheres of radius R and R + 0.05: every distance lies between 0.05 - s and 0.05 + s, s = the
    # sagitta of the outer one (how far its faces dip below its vertices' sphere), computed from the mesh
    C, R, gap = np.array([0.07, -0.05, 0.03]), 0.55, 0.05
    inner, outer = O.icosphere(2, C, R), O.icosphere(2, C, R + gap)
    s = (R + gap) - Q.query(C[None], *outer)[0][0]
    assert 0.005 < s < 0.02
    e = MQ.mesh_error(inner, outer, n=4000, seed=2)
    print('mesh_error(R, R + 0.05): sagitta %.5f' % s, e)
    for side in ('a_to_b', 'b_to_a'):
        assert gap - s <= e[side]['mean'] <= gap + s
        assert e[side]['mean'] <= e[side]['rms'] <= e[side]['max'] <= gap + s + 1e-6
    signed = MQ.mesh_error(inner, outer, n=4000, seed=2, signed=True)
    assert signed['a_to_b']['mean'] == -e['a_to_b']['mean'] and signed['b_to_a']['mean'] == e['b_to_a']['mean']


def test_surface_scores_exact(cases):
    from octfusion_amd import recon_metrics as RM
    m = to_dev(cases['sphere']['mesh'])
    other = to_dev(O.icosphere(2, (0.07, -0.05, 0.03), 0.6))
    taus = (0.03, 0.07)                                          # the gap 0.05 -+ the sagitta, about 0.01
    before = RM.surface_scores(m, other, n=3000, seed=4, thresholds=taus)
    s = RM.surface_scores(m, m, n=3000, seed=4, exact=True)
    print('exact scores of a mesh against itself:', s)
    assert s['fscore'] == [1.0, 1.0, 1.0] and s['chamfer_l1'] <= 1e-6 and s['chamfer_l2'] <= 1e-12
    assert s['normal_consistency'] >= 1 - 1e-3         # the nearest face is the sample's own, but for ties on an edge
    e = RM.surface_scores(m, other, n=3000, seed=4, thresholds=taus, exact=True)
    assert 0.04 < e['completeness'] < 0.06 and 0.04 < e['accuracy'] < 0.06 and e['fscore'] == [0.0, 1.0]
    assert e['normal_consistency'] > 0.85              # the face across the gap, or one that shares a vertex with it
    # the default path is what it was: the same dict before and after the exact calls, and with exact=False spelt out
    assert RM.surface_scores(m, other, n=3000, seed=4, thresholds=taus) == before
    assert RM.surface_scores(m, other, n=3000, seed=4, thresholds=taus, exact=False) == before
    cloud = (torch.rand(50, 3, device=dev()), torch.nn.functional.normalize(torch.rand(50, 3, device=dev()), dim=1))
    with pytest.raises(ValueError, match='exact=True needs'):
        RM.surface_scores(m, cloud, n=100, exact=True)


def test_command_lines(tmp_path, cases):
    from octfusion_amd import mesh
    a, b = str(tmp_path / 'a.obj'), str(tmp_path / 'b.obj')
    C = (0.07, -0.05, 0.03)
    mesh.write_obj(a, *O.icosphere(3, C, 0.55))
    mesh.write_obj(b, *O.icosphere(3, C, 0.6))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, '-m', 'octfusion_amd.mesh_query', '--a', a, '--b', b, '--samples', '2000',
                          '--signed'], capture_output=True, text=True, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    e = json.loads(out.stdout.strip().splitlines()[-1])
    assert e['samples'] == 2000 and 0.045 < e['hausdorff'] < 0.055
    assert -0.055 < e['a_to_b']['mean'] < -0.045 and 0.045 < e['b_to_a']['mean'] < 0.055     # a lies inside b
    out = subprocess.run([sys.executable, '-m', 'octfusion_amd.simplify', '--input', a, '--out', str(tmp_path / 's'),
                          '--cells', '8', '--error', '2000'], capture_output=True, text=True, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r['faces_out'][0] < r['faces_in'][0] == 1280 and len(r['error']) == 1
    assert 0 < r['error'][0]['hausdorff'] < 3 ** 0.5 * 1.1 / 8          # a vertex moves within its cell of the grid
    assert r['error'][0]['samples'] == 2000


def test_reconstruct_scores_exact(golden, tmp_path):
    """reconstruct(metrics=True, exact=True) on a mesh input (the tiny VAE of test_gpu_reconstruct.py, random weights):
    the record is surface_scores(gt mesh in the output frame, reconstruction, exact=True); without `exact` it is what
    it was."""
    from octfusion_amd import mesh, reconstruct as R, recon_metrics as RM, synthetic
    from octfusion_amd.graph_vae import GraphVAE
    kw = {k: v for k, v in golden('g_vae_enc')['cfg'].items()}
    path = str(tmp_path / 'ball.obj')
    mesh.write_obj(path, *O.icosphere(3, (0.0, 0.0, 0.0), 0.7))
    vae = GraphVAE(**kw)
    vae.load_state_dict(synthetic.random_state_dict(vae))
    vae = vae.to(dev()).eval()
    cfg = {'depth': kw['depth'], 'full_depth': kw['full_depth'], 'point_scale': 0.5}
    inputs = R.read_inputs([path], from_mesh=True)
    args = dict(sdf_resolution=32, batch=1, seed=4, points=4000, chamfer_points=2048, metrics=True,
                thresholds=(0.02, 0.05))
    plain = R.reconstruct(vae, cfg, inputs, dev(), **args)
    exact = R.reconstruct(vae, cfg, inputs, dev(), exact=True, **args)
    again = R.reconstruct(vae, cfg, inputs, dev(), exact=False, **args)
    assert again['shapes'] == plain['shapes']
    (v, f), rec = exact['meshes']['ball'], exact['shapes']['ball']
    assert f.shape[0] > 0 and set(rec) == set(plain['shapes']['ball'])
    assert {k: x for k, x in rec.items() if k != 'scores'} == {k: x for k, x in plain['shapes']['ball'].items()
                                                               if k != 'scores'}
    gv = torch.from_numpy(inputs[0]['verts']).to(dev())
    c, s = R._frame(gv)
    gt = ((gv - c) * (s * 0.9 * 0.5), torch.from_numpy(inputs[0]['faces']).to(dev()))
    assert rec['scores'] == RM.surface_scores(gt, (v, f), n=2048, seed=4, thresholds=(0.02, 0.05), exact=True)
    assert rec['scores'] != plain['shapes']['ball']['scores']
    # measured against triangles, a sample is never farther than from the nearest sample of the same surface
    assert rec['scores']['accuracy'] <= plain['shapes']['ball']['scores']['accuracy'] + 1e-6
    assert rec['scores']['completeness'] <= plain['shapes']['ball']['scores']['completeness'] + 1e-6
