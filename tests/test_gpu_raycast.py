"""GPU tests of the ray casts (csrc/ofx_raycast.hip, octfusion_amd/raycast.py) against the float64 oracle
(tests/raycast_oracle.py: the contract by brute force, and an independent Moeller-Trumbore intersection).

Shapes and ray sets: raycast_oracle.shapes() / ray_sets() -- box 12 faces, icospheres of 320 and 5120, torus 256, plate
2; per shape 4096 rays (1024 on the 5120-face sphere), half aimed at the mesh from the sphere of radius 2, half from
random origins in [-1.2, 1.2]^3 in random directions, direction lengths in [0.5, 2].  tests/test_raycast_oracle.py
establishes on the CPU that no ray of these sets has a margin below 1e-6 (1 % would be allowed) and that the contract
oracle reports no miss from the interior origins.

Tolerances.
  t       hit / miss equal to the contract oracle's on every ray above the margin; |t - t_MT| <= 2^-22 |t| against the
          independent oracle: both sides compute in fp64 from the same fp32 inputs (the two fp64 results agree to
          8e-15, measured on the CPU) and the device rounds once to fp32, 2^-24 |t|.  Measured maximum: 5.92e-8.
  faces   never compared by index across formulations except where the margin allows it: the oracle's own t of the
          RETURNED face is within the same tolerance of the minimum.
  point   |org + t dir - point| <= 2^-22 (|org| + |t dir| + |point|) (max norms): t, the product and the point are each
          rounded to fp32 once; closest_point(point).dist <= 2^-20 x the diagonal of the mesh's box.
  frames  a mesh scaled by 40 and moved to (100, -50, 7) is rounded to fp32 at magnitude <= 150: half an ulp, 3.8e-6,
          is 1e-7 in the unit frame, and the direction x 40 is rounded too (6e-8 x a distance <= 3): together
          a few 1e-6 of a triangle's height (>= 0.1).  Faces are compared on rays whose
          margin is >= 1e-4, well above that.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import raycast_oracle as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['box', 'sphere', 'sphere4', 'torus', 'plate']
TOL = 2.0 ** -22


def dev():
    return torch.device('cuda:0')


def to_dev(m):
    v, f = m
    return (torch.from_numpy(np.asarray(v, np.float32)).to(dev()), torch.from_numpy(np.asarray(f, np.int32)).to(dev()))


def f32_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).reshape(-1, 3).to(dev())


def run(meshes, orgs, dirs, **kw):
    """ray_cast on numpy meshes and rays -> per mesh (t fp32, face int32, point fp32 or None, cos fp32 or None)."""
    from octfusion_amd import raycast as RC
    out = RC.ray_cast([to_dev(m) for m in meshes], [f32_dev(o) for o in orgs], [f32_dev(d) for d in dirs], **kw)
    assert len(out) == len(meshes)
    res = []
    for (t, f, p, c), o in zip(out, orgs):
        n = len(o)
        assert t.shape == (n,) and t.dtype == torch.float32 and f.shape == (n,) and f.dtype == torch.int32
        assert (p is None) == (kw.get('want_point', True) is False) and (c is None) == (kw.get('want_cos', True) is False)
        assert p is None or (p.shape == (n, 3) and p.dtype == torch.float32)
        assert c is None or (c.shape == (n,) and c.dtype == torch.float32)
        res.append((t.cpu().numpy(), f.cpu().numpy(), None if p is None else p.cpu().numpy(),
                    None if c is None else c.cpu().numpy()))
    return res


def same(a, b):
    """Bitwise equality of two result tuples (NaNs included)."""
    return all((x is None and y is None) or np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def cut(res, sl):
    return tuple(None if x is None else x[sl] for x in res)


@pytest.fixture(scope='module')
def scenes():
    meshes, sets = dict(R.shapes()), R.ray_sets()
    out = {}
    for n in NAMES:
        (V, F), (o, d) = meshes[n], sets[n]
        out[n] = dict(mesh=(V, F), org=o, dir=d, cast=R.cast(o, d, V, F), mt=R.moller_trumbore(o, d, V, F)[0])
    return out


@pytest.fixture(scope='module')
def results(scenes):
    """The device results of the five shapes: one call, shared."""
    return dict(zip(NAMES, run([scenes[n]['mesh'] for n in NAMES], [scenes[n]['org'] for n in NAMES],
                               [scenes[n]['dir'] for n in NAMES])))


# ---- 1 values -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_values(name, scenes, results):
    s, (t, face, point, cosn) = scenes[name], results[name]
    c = s['cast']
    ok = c['margin'] >= R.MARGIN
    hit = np.isfinite(c['t'])
    assert (~ok).sum() <= 0.01 * len(ok)
    assert np.array_equal(np.isfinite(t)[ok], hit[ok]) and np.array_equal((face >= 0), np.isfinite(t))
    assert (np.isposinf(t) | np.isfinite(t)).all()
    both = ok & hit
    rel = np.abs(t[both].astype(np.float64) - s['mt'][both]) / np.abs(s['mt'][both])
    print('%s: %d rays, %d hits, %d left out; max |t - t_MT| / |t| = %.3e (2^-24 = 5.96e-8)'
          % (name, len(t), hit.sum(), (~ok).sum(), rel.max()))
    assert rel.max() <= TOL
    print('%s: %d of %d values differ in a bit from the contract oracle rounded to fp32'
          % (name, (t[both] != c['t'][both].astype(np.float32)).sum(), both.sum()))


# ---- 2 faces, tie-proof -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_face(name, scenes, results):
    s, (t, face, _, _) = scenes[name], results[name]
    c = s['cast']
    hit = face >= 0
    assert face[hit].max() < len(s['mesh'][1])
    rows = np.nonzero(hit)[0]
    own = c['pair_t'][rows, face[rows]]
    assert c['pair_hit'][rows, face[rows]].all()                # the oracle, too, says the ray meets the returned face
    assert (np.abs(own - c['t'][rows]) <= TOL * np.abs(c['t'][rows])).all()
    ok = c['margin'] >= R.MARGIN
    print('%s: %d of %d face indices differ from the oracle\'s' % (name, (face != c['face'])[ok].sum(), ok.sum()))


def test_the_lower_face_on_a_diagonal(scenes):
    box = scenes['box']['mesh']
    org = np.array([[0.25, 0.25, -2.0], [-0.125, -0.125, -2.0], [0.1, 0.3, -2.0], [0.3, 0.1, -2.0], [0.5, 0.1, -2.0],
                    [0.5, 0.5, -2.0], [0.6, 0.0, -2.0]])
    d = np.tile([0.0, 0.0, 1.0], (len(org), 1))
    t, face, point, cosn = run([box], [org], [d])[0]
    assert (t[:6] == 1.5).all() and np.isposinf(t[6]) and face[6] == -1       # diagonal, edge and corner do not leak
    assert face[:4].tolist() == [8, 8, 8, 9]                     # faces 8 and 9 share the diagonal: the lower one
    assert np.array_equal(point[:4], np.concatenate([org[:4, :2], np.full((4, 1), -0.5)], 1).astype(np.float32))
    assert (cosn[:4] == -1.0).all()


# ---- 3 point and cosine -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_point_and_cosine(name, scenes, results):
    from octfusion_amd import mesh_query as MQ
    s, (t, face, point, cosn) = scenes[name], results[name]
    V, F = s['mesh']
    hit = face >= 0
    assert np.isnan(point[~hit]).all() and np.isnan(cosn[~hit]).all()
    o, d = s['org'][hit], s['dir'][hit]
    along = t[hit].astype(np.float64)[:, None] * d
    err = np.abs(o + along - point[hit]).max(1)
    scale = np.abs(o).max(1) + np.abs(along).max(1) + np.abs(point[hit]).max(1)
    print('%s: max |org + t dir - point| = %.3e' % (name, err.max()))
    assert (err <= TOL * scale).all()
    dist = MQ.closest_point([to_dev((V, F))], [torch.from_numpy(point[hit]).to(dev())], want_point=False)[0][0]
    extent = np.linalg.norm(V.max(0) - V.min(0))
    print('%s: hit points are at most %.3e off the mesh (extent %.3f)' % (name, float(dist.max()), extent))
    assert float(dist.max()) <= 2.0 ** -20 * extent
    ok = (s['cast']['margin'] >= R.MARGIN) & hit
    assert np.abs(cosn[ok] - s['cast']['cos'][ok]).max() <= 1e-6
    assert (np.abs(cosn[hit]) <= 1.0).all()
    if name in ('sphere', 'sphere4'):                            # the winding: negative from outside, positive from inside
        r = np.linalg.norm(s['org'] - np.array([0.07, -0.05, 0.03]), axis=1)
        outside, inside = hit & (r > 0.56), hit & (r < 0.5)
        assert outside.sum() > 100 and inside.sum() > 10
        assert (cosn[outside] < 0).all() and (cosn[inside] > 0).all()


# ---- 4 watertightness ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', R.CLOSED)
def test_no_ray_leaks_out_of_a_closed_mesh(name, scenes):
    V, F = scenes[name]['mesh']
    org, d = R.interior_rays(name, V, F)
    t, face, _, _ = run([(V, F)], [org], [d], want_point=False, want_cos=False)[0]
    print('%s: %d rays towards vertices, edge midpoints and hashed directions, %d misses' % (name, len(t),
                                                                                           (face < 0).sum()))
    assert (face >= 0).all() and np.isfinite(t).all() and (t > 0).all()


# ---- 5 purity -----------------------------------------------------------------------------------------------------
def test_order_bins_and_batch_do_not_change_a_bit(scenes, results):
    rng = np.random.default_rng(11)
    for name in ('torus', 'box'):
        s, want = scenes[name], results[name]
        perm = rng.permutation(len(s['org']))
        got = run([s['mesh']], [s['org'][perm]], [s['dir'][perm]])[0]
        assert same(got, cut(want, perm)), (name, 'permutation')
        for bins in (1, 3, 16, 0):
            assert same(run([s['mesh']], [s['org']], [s['dir']], bins=bins)[0], want), (name, bins)
        assert same(run([s['mesh']], [s['org']], [s['dir']], coherent=True)[0], want), (name, 'coherent')
    s4 = scenes['sphere4']
    for bins in (1, 2, 16):
        assert same(run([s4['mesh']], [s4['org']], [s4['dir']], bins=bins)[0], results['sphere4']), bins
    # alone against a batch of three shapes with different ray counts, one of them zero
    a, b, c = scenes['sphere'], scenes['plate'], scenes['torus']
    got = run([a['mesh'], b['mesh'], c['mesh']], [a['org'][:1000], np.zeros((0, 3)), c['org'][:777]],
              [a['dir'][:1000], np.zeros((0, 3)), c['dir'][:777]])
    assert same(got[0], cut(results['sphere'], slice(0, 1000)))
    assert got[1][0].shape == (0,) and got[1][2].shape == (0, 3)
    assert same(got[2], cut(results['torus'], slice(0, 777)))


def test_a_mesh_in_another_frame(scenes, results):
    s = scenes['torus']
    V, F = s['mesh']
    shift = np.array([100.0, -50.0, 7.0])
    t, face, point, cosn = run([(V * 40 + shift, F)], [s['org'] * 40 + shift], [s['dir'] * 40])[0]
    clear = s['cast']['margin'] >= 1e-4
    print('moved torus: %d of %d rays are clear of every edge by 1e-4' % (clear.sum(), len(clear)))
    assert clear.sum() >= 0.95 * len(clear)
    assert np.array_equal(face[clear], results['torus'][1][clear])
    hit = clear & (face >= 0)
    assert np.abs(t[hit] - results['torus'][0][hit]).max() <= 1e-4          # the same parameter: rays moved alike


@pytest.mark.parametrize('n', [1, 63, 64, 65])
def test_ray_counts_around_a_wave(n, scenes, results):
    s = scenes['sphere']
    sl = slice(3000, 3000 + n)
    assert same(run([s['mesh']], [s['org'][sl]], [s['dir'][sl]])[0], cut(results['sphere'], sl))


# ---- 6 range and rejects ------------------------------------------------------------------------------------------
def test_windows_of_t(scenes):
    box = scenes['box']['mesh']
    o, d = np.array([[0.1, 0.2, -2.0]]), np.array([[0.0, 0.0, 1.0]])
    on = np.array([[0.1, 0.2, -0.5]])

    def t_of(org, dr, **kw):
        return float(run([box], [org], [dr], want_point=False, want_cos=False, **kw)[0][0][0])
    assert t_of(o, d) == 1.5 and t_of(o, 2 * d) == 0.75
    assert t_of(o, d, tmin=1.6) == 2.5 and t_of(o, d, tmin=2.6) == np.inf
    assert t_of(o, d, tmax=1.5) == 1.5                                        # a hit exactly at tmax
    assert t_of(o, d, tmax=float(np.nextafter(np.float32(1.5), np.float32(0)))) == np.inf
    assert t_of(o, -d) == np.inf and t_of(o, -d, tmin=-np.inf, tmax=0.0) == -2.5
    assert t_of(on, d) == 0.0 and t_of(on, d, tmin=1e-3) == 1.0               # a ray that starts on the surface
    s = scenes['torus']
    for kw in (dict(tmin=0.8, tmax=1.7), dict(tmin=-np.inf, tmax=np.inf)):
        want = R.cast(s['org'], s['dir'], *s['mesh'], **kw)
        t, face, _, _ = run([s['mesh']], [s['org']], [s['dir']], **kw)[0]
        near = np.isfinite(want['pair_t']) & ((np.abs(want['pair_t'] - 0.8) < 1e-5) | (np.abs(want['pair_t'] - 1.7) < 1e-5))
        ok = (want['margin'] >= R.MARGIN) & ~near.any(1)                      # no hit within 1e-5 of a window's end
        assert ok.sum() >= 0.99 * len(ok)
        assert np.array_equal(np.isfinite(t)[ok], np.isfinite(want['t'])[ok])
        hit = ok & np.isfinite(want['t'])
        assert (np.abs(t[hit] - want['t'][hit]) <= TOL * np.abs(want['t'][hit])).all()


def test_rays_that_are_refused(scenes, results):
    s = scenes['sphere']
    o, d = s['org'][:300].copy(), s['dir'][:300].copy()
    bad = [0, 7, 63, 64, 100, 299]
    o[0] = [np.nan, 0, 0]
    d[7] = [0, np.inf, 0]
    d[63] = [0, 0, 0]
    o[64] = [np.nan, np.nan, np.nan]
    d[100] = [np.inf, np.nan, 0.1]
    o[299] = [0.2, -np.inf, 0.1]
    good = np.setdiff1d(np.arange(300), bad)
    t, face, point, cosn = run([s['mesh']], [o], [d])[0]
    assert np.isposinf(t[bad]).all() and (face[bad] == -1).all() and np.isnan(point[bad]).all()
    assert np.isnan(cosn[bad]).all()
    assert same((t[good], face[good], point[good], cosn[good]), cut(results['sphere'], good))
    t, face, point, cosn = run([s['mesh']], [np.full((70, 3), np.nan)], [np.zeros((70, 3))])[0]
    assert np.isposinf(t).all() and (face == -1).all() and np.isnan(point).all() and np.isnan(cosn).all()
    # directions outside the range in which 1 / d is safe in fp32 are answered all the same (never culled): scaling by
    # a power of two is exact, so t scales and nothing else moves
    tiny = run([s['mesh']], [s['org'][:128]], [s['dir'][:128] * 2.0 ** -104])[0]
    want = cut(results['sphere'], slice(0, 128))
    assert np.array_equal(tiny[1], want[1]) and same(tiny[2:], want[2:])
    assert np.array_equal(tiny[0], want[0] * np.float32(2.0 ** 104))


def test_degenerate_and_doubled_faces(scenes, results):
    s = scenes['torus']
    V, F = s['mesh']
    twice = (V, np.concatenate([F, F]))
    assert same(run([twice], [s['org']], [s['dir']])[0], results['torus'])
    n = len(V)
    more = (np.concatenate([V, [[0.0, 0.0, 0.0], [0.3, 0.0, 0.0], [0.6, 0.0, 0.0]]]),
            np.concatenate([[[n, n + 1, n + 2], [n, n, n]], F]).astype(np.int32))       # a segment and a point in front
    t, face, point, cosn = run([more], [s['org']], [s['dir']])[0]
    want = results['torus']
    assert np.array_equal(face, np.where(want[1] >= 0, want[1] + 2, -1))
    assert same((t, point, cosn), (want[0], want[2], want[3]))


def raw_cast(meshes, orgs, dirs, bins=0, tmin=0.0, tmax=np.inf):
    """ofx_ray_cast itself: (return code, status, t, face) with the outputs prefilled with a sentinel."""
    from octfusion_amd import _lib
    vs = torch.cat([to_dev(m)[0] for m in meshes])
    fs = torch.cat([to_dev(m)[1] for m in meshes])
    o, d = torch.cat([f32_dev(x) for x in orgs]), torch.cat([f32_dev(x) for x in dirs])
    nv, nf, nq = [len(m[0]) for m in meshes], [len(m[1]) for m in meshes], [len(x) for x in orgs]
    offs = torch.from_numpy(np.stack([np.cumsum([0] + nv), np.cumsum([0] + nf), np.cumsum([0] + nq)])).to(dev())
    B, Q = len(meshes), sum(nq)
    nbytes = _lib.lib().ofx_ray_cast_ws_bytes(B, sum(nv), sum(nf), Q, bins if 0 <= bins <= 16 else 0)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev())
    t = torch.full((Q,), 77.0, device=dev())
    face = torch.full((Q,), 77, dtype=torch.int32, device=dev())
    status = torch.full((B,), 77, dtype=torch.int32, device=dev())
    rc = _lib.lib().ofx_ray_cast(vs.data_ptr(), fs.data_ptr(), offs[0].data_ptr(), offs[1].data_ptr(), o.data_ptr(),
                                 d.data_ptr(), offs[2].data_ptr(), B, Q, max(nq), tmin, tmax, bins, 0, t.data_ptr(),
                                 face.data_ptr(), None, None, ws.data_ptr(), status.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    cuts = np.cumsum(nq)[:-1]
    return rc, status.cpu().numpy(), np.split(t.cpu().numpy(), cuts), np.split(face.cpu().numpy(), cuts)


def test_a_bad_shape_is_refused_alone(scenes, results):
    from octfusion_amd import raycast as RC
    s, t = scenes['sphere'], scenes['torus']
    V, F = t['mesh']
    bad_index = (V, F.copy())
    bad_index[1][17, 1] = len(V)
    nan_vertex = (V.copy(), F)
    nan_vertex[0][F[40, 2], 0] = np.nan
    for bad in (bad_index, nan_vertex):
        rc, status, tt, face = raw_cast([s['mesh'], bad, s['mesh']], [s['org'][:200], t['org'][:100], s['org'][:50]],
                                        [s['dir'][:200], t['dir'][:100], s['dir'][:50]])
        assert rc == 0 and status.tolist() == [0, 1, 0]
        assert (tt[1] == 77).all() and (face[1] == 77).all()                  # left unwritten
        want = results['sphere']
        assert np.array_equal(tt[0], want[0][:200]) and np.array_equal(face[0], want[1][:200])
        assert np.array_equal(tt[2], want[0][:50]) and np.array_equal(face[2], want[1][:50])
        with pytest.raises(ValueError, match='shape 1 has a face index outside'):
            RC.ray_cast([to_dev(s['mesh']), to_dev(bad), to_dev(s['mesh'])], [f32_dev(s['org'][:8])] * 3,
                        [f32_dev(s['dir'][:8])] * 3)


def test_wrong_arguments_raise_before_a_launch(scenes):
    from octfusion_amd import _lib, raycast as RC
    box = scenes['box']
    m, o, d = to_dev(box['mesh']), f32_dev(box['org'][:10]), f32_dev(box['dir'][:10])
    for bins in (-1, 17):
        with pytest.raises(ValueError, match='bins'):
            RC.ray_cast([m], [o], [d], bins=bins)
    with pytest.raises(ValueError, match='float32'):
        RC.ray_cast([m], [o.double()], [d])
    with pytest.raises(ValueError, match='float32'):
        RC.ray_cast([m], [o], [d.half()])
    with pytest.raises(ValueError, match='float32 vertices and int32 faces'):
        RC.ray_cast([(m[0], m[1].long())], [o], [d])
    with pytest.raises(ValueError, match=r'\[n, 3\]'):
        RC.ray_cast([m], [o[:, :2]], [d])
    with pytest.raises(ValueError, match=r'\[B, n, 3\]'):
        RC.ray_cast([m], o, [d])
    with pytest.raises(ValueError, match='2 sets of origins for 1 meshes'):
        RC.ray_cast([m], [o, o], [d, d])
    with pytest.raises(ValueError, match='10 origins for 9 directions'):
        RC.ray_cast([m], [o], [d[:9]])
    with pytest.raises(ValueError, match='not on the device'):
        RC.ray_cast([m], [o.cpu()], [d])
    with pytest.raises(ValueError, match='shape 0 has no faces'):
        RC.ray_cast([(m[0], m[1][:0])], [o], [d])
    with pytest.raises(ValueError, match='no meshes'):
        RC.ray_cast([], [], [])
    with pytest.raises(ValueError, match='NaN'):
        RC.ray_cast([m], [o], [d], tmin=float('nan'))
    stacked = RC.ray_cast([m, m], torch.stack([o, o]), torch.stack([d, d]))
    assert torch.equal(stacked[0][0], stacked[1][0]) and stacked[0][2].shape == (10, 3)
    # the C entry refuses what the wrapper would not pass on
    L = _lib.lib()
    assert L.ofx_ray_cast_ws_bytes(1, 8, 12, 10, 17) == 0 and L.ofx_ray_cast_ws_bytes(0, 8, 12, 10, 0) == 0
    assert L.ofx_ray_cast_ws_bytes(1, 8, 12, -1, 0) == 0 and L.ofx_ray_cast_ws_bytes(1, 8, 0, 10, 0) == 0
    assert L.ofx_ray_cast_ws_bytes(1, 8, 12, 2 ** 30 + 1, 0) == 0 and L.ofx_ray_scan_ws_bytes(-1) == 0
    small, big = L.ofx_ray_cast_ws_bytes(1, 8, 12, 10, 4), L.ofx_ray_cast_ws_bytes(1, 8, 1012, 10, 4)
    assert 1000 * 40 - 256 <= big - small <= 1000 * 40 + 256                  # 36 + 4 bytes per face
    for kw in (dict(bins=17), dict(bins=-1), dict(tmin=float('nan'))):
        rc, status, t, face = raw_cast([box['mesh']], [box['org'][:10]], [box['dir'][:10]], **kw)
        assert rc == -1 and status.tolist() == [77] and (t[0] == 77).all() and (face[0] == 77).all()


def test_workspace_sizes_are_those_of_the_separate_builders():
    """ofx_mesh_query and ofx_ray_cast carve one layout (ofx_tribins_layout).  The literals are what each entry returned
    for (batch, verts, faces, items, bins) on an MI355X while it still had a layout of its own (the sort's share, which
    weighs in the last one, is the device's answer): a caller's workspace stays valid."""
    from octfusion_amd import _lib
    L = _lib.lib()
    for args, nbytes in (((1, 8, 12, 10, 0), 150272), ((1, 8, 12, 10, 4), 5120), ((3, 100, 1000, 0, 1), 41984),
                         ((2, 50000, 100000, 1000000, 16), 40303616)):
        assert L.ofx_mesh_query_ws_bytes(*args) == nbytes, args
        assert L.ofx_ray_cast_ws_bytes(*args) == nbytes, args
        assert L.ofx_mesh_query_ws_bytes(*args) == L.ofx_ray_cast_ws_bytes(*args)


# ---- 7 culling ----------------------------------------------------------------------------------------------------
def test_culling_happens(scenes, results):
    from octfusion_amd import _lib
    s = scenes['sphere4']
    words = torch.zeros(3, dtype=torch.int64, device=dev())
    _lib.call('ofx_ray_cast_set_counters', words.data_ptr())
    try:
        got = run([s['mesh']], [s['org']], [s['dir']])[0]
        torch.cuda.synchronize()
    finally:
        _lib.call('ofx_ray_cast_set_counters', None)
    bins, staged, pairs = words.tolist()
    full = len(s['org']) * len(s['mesh'][1])
    print('5120-face sphere, %d rays, automatic bins: %d bins visited, %d triangles staged, %d pairs of %d (%.2f %%)'
          % (len(s['org']), bins, staged, pairs, full, 100.0 * pairs / full))
    assert same(got, results['sphere4'])
    assert 0 < pairs < full and bins > 0 and staged > 0


# ---- 8 images -----------------------------------------------------------------------------------------------------
def test_ray_images(scenes):
    """ray_images at size 32 on the 320-face sphere from the 20 FID views.  The face image against the rasteriser's
    (render(buffers=True), samples = 1): the two differ by design near edges, where the rasteriser snaps to 1/256
    pixel.  Between the two CPU oracles 8 of 20 480 pixels differ (3.9e-4; raycast_oracle.IMAGE_MISMATCH, asserted in
    tests/test_raycast_oracle.py); the device is allowed twice that, 16.  Measured on the device: 8 of 20 480."""
    from octfusion_amd import raycast as RC, render
    V, F = scenes['sphere']['mesh']
    S = 32
    img = RC.ray_images([(V, F)], size=S)
    depth, face, point, normal = (img[k][0].cpu().numpy() for k in ('depth', 'face', 'point', 'normal'))
    assert depth.shape == (20, S, S) and depth.dtype == np.float32 and face.shape == (20, S, S)
    assert face.dtype == np.int32 and point.shape == (20, S, S, 3) and normal.shape == (20, S, S, 3)
    assert normal.dtype == np.uint8
    bg = face < 0
    assert 0.2 < bg.mean() < 0.8
    assert np.isposinf(depth[bg]).all() and (normal[bg] == 255).all() and np.isnan(point[bg]).all()
    assert np.isfinite(depth[~bg]).all() and bg[:, 0, 0].all() and not bg[:, 16, 16].any()
    # the centre pixel: camera distance minus the radius, to the faceting error (the pixel's centre is half a pixel
    # off the axis: a sagitta of 4e-4 at most, inside the 2e-3 allowed on top)
    Vn = R.unit_frame(V)
    n = np.cross(Vn[F[:, 1]] - Vn[F[:, 0]], Vn[F[:, 2]] - Vn[F[:, 0]])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    rmax, rmin = np.linalg.norm(Vn, axis=1).max(), np.abs(np.einsum('ik,ik->i', n, Vn[F[:, 0]])).min()
    eye = np.linalg.norm(render.fid_views(), axis=1)
    assert 0.9 < rmin < rmax <= 1.0 + 1e-6
    assert (depth[:, 16, 16] >= eye - rmax - 2e-3).all() and (depth[:, 16, 16] <= eye - rmin + 2e-3).all()
    # the normal map decodes to the hit faces' normals turned towards the camera
    dec = normal[~bg].astype(np.float64) / 255.0 * 2.0 - 1.0
    want = n[face[~bg]]
    view = np.broadcast_to(render.fid_views()[:, None, None, :], point.shape)[~bg] - point[~bg]
    want = np.where((np.einsum('ik,ik->i', want, view) < 0)[:, None], -want, want)
    assert np.abs(dec - want).max() <= 1.0 / 127.0
    # hit points lie on their rays at the depth: point = eye + depth * R (u, v, -1), so (point - eye) . forward = depth
    fwd = -render.fid_views() / eye[:, None]
    along = np.einsum('vijk,vk->vij', point - render.fid_views()[:, None, None, :], fwd)
    assert np.abs(along[~bg] - depth[~bg]).max() <= 1e-5
    # against the rasteriser
    _, buf = render.render([(V, F)], size=S, buffers=True)
    ids = buf['ids'][0].cpu().numpy()
    differ = int((ids != face).sum())
    print('ray_images against render: %d of %d face ids differ (the CPU oracles: %d)' % (differ, face.size,
                                                                                        R.IMAGE_MISMATCH))
    assert differ <= 2 * R.IMAGE_MISMATCH
    # camera_rays are the oracle's rays in tile order, with the inverse permutation
    pose = render.fid_poses()[3]
    o, d, inv = RC.camera_rays(pose, 11)
    ro, rd = R.camera_rays(pose, 11)
    assert np.array_equal(o.cpu().numpy()[inv.cpu().numpy()], ro.astype(np.float32))
    assert np.array_equal(d.cpu().numpy()[inv.cpu().numpy()], rd.astype(np.float32))
    perm, _ = RC.tile_order(11)
    assert perm[:9].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 11] and perm[64:68].tolist() == [8, 9, 10, 19]


# ---- 9 scans ------------------------------------------------------------------------------------------------------
def test_virtual_scan(scenes, tmp_path):
    from octfusion_amd import mesh, mesh_query as MQ, normals, raycast as RC, render
    V, F = scenes['sphere']['mesh']
    m = to_dev((V, F))
    extent = np.linalg.norm(V.max(0) - V.min(0))
    poses = render.fid_poses()
    # one pose: only what faces the camera
    (p, n), = RC.virtual_scan([m], poses[:1], size=48)
    assert p.dtype == torch.float32 and n.dtype == torch.float32 and p.shape == n.shape and p.shape[1] == 3
    img = RC.ray_images([m], poses[:1], size=48, normalize=False)
    hits = (img['face'][0, 0] >= 0)
    assert p.shape[0] == int(hits.sum()) > 100
    assert float((p - img['point'][0, 0][hits]).abs().max()) <= 1e-6      # view then row-major pixel order
    eye = torch.from_numpy(render.fid_views()[0]).to(dev())
    assert bool(((n.double() * (eye - p.double())).sum(1) > 0).all())
    assert float((n.double().norm(dim=1) - 1).abs().max()) <= 1e-6
    # 20 poses, two meshes: every point is on its mesh; two runs are bit-equal
    T = to_dev(scenes['torus']['mesh'])
    a = RC.virtual_scan([m, T], poses, size=24)
    b = RC.virtual_scan([m, T], poses, size=24)
    for (pa, na), (pb, nb), msh in zip(a, b, (m, T)):
        assert pa.shape[0] > 1000 and torch.equal(pa, pb) and torch.equal(na, nb)
        dist = MQ.closest_point([msh], [pa.contiguous()], want_point=False)[0][0]
        assert float(dist.max()) <= 2.0 ** -20 * 2.0
    # noise: along the ray, Gaussian, reproducible, different per seed
    (pn, nn), = RC.virtual_scan([m], poses[:4], size=48, noise=0.01, seed=3)
    (pn2, _), = RC.virtual_scan([m], poses[:4], size=48, noise=0.01, seed=3)
    (pn3, _), = RC.virtual_scan([m], poses[:4], size=48, noise=0.01, seed=4)
    (pc, nc), = RC.virtual_scan([m], poses[:4], size=48)
    assert torch.equal(pn, pn2) and torch.equal(nn, nc) and not torch.equal(pn, pn3) and pn.shape == pc.shape
    move = (pn - pc).double()
    size = move.norm(dim=1)
    assert 0.009 < float(size.pow(2).mean().sqrt()) < 0.011 and abs(float(move.mean())) < 1e-3
    # the files: a .ply that normals.read_cloud reads back
    path = str(tmp_path / 'scan.ply')
    mesh.write_ply(path, p, n)
    assert np.array_equal(normals.read_cloud(path), p.cpu().numpy())
    assert np.array_equal(mesh.read_ply(path)[1], n.cpu().numpy())


def test_command_line(tmp_path, scenes):
    from octfusion_amd import mesh, normals
    obj = str(tmp_path / 'ball.obj')
    mesh.write_obj(obj, *scenes['sphere']['mesh'])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, '-m', 'octfusion_amd.raycast', '--input', obj, '--out', str(tmp_path / 'o'),
                          '--views', '3', '--size', '32', '--noise', '0.002', '--normal-maps'],
                         capture_output=True, text=True, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    assert rec['shapes'] == 1 and rec['views'] == 3 and rec['points']['ball'] > 500
    pts, nrm = mesh.read_ply(str(tmp_path / 'o' / 'ball.ply'))
    assert len(pts) == rec['points']['ball'] == len(normals.read_cloud(str(tmp_path / 'o' / 'ball.ply')))
    assert np.abs(np.linalg.norm(pts, axis=1) - 1.0).max() < 0.05 and np.abs(np.linalg.norm(nrm, axis=1) - 1).max() < 1e-5
    for j in range(3):
        png = open(str(tmp_path / 'o' / ('view_%d' % j) / 'ball.png'), 'rb').read()
        assert png[:8] == b'\x89PNG\r\n\x1a\n' and len(png) > 200
