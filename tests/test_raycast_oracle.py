"""CPU checks of the ray-cast oracle (tests/raycast_oracle.py): the contract agrees with an independent
Moeller-Trumbore intersection and with analytic cases, and the reference alone satisfies the facts
tests/test_gpu_raycast.py leans on (few rays near a triangle boundary; no miss from inside a closed mesh)."""
import numpy as np
import pytest

import raycast_oracle as R


@pytest.fixture(scope='module')
def scenes():
    meshes = dict(R.shapes())
    sets = R.ray_sets()
    return {n: dict(mesh=meshes[n], rays=sets[n], cast=R.cast(*sets[n], *meshes[n]),
                    mt=R.moller_trumbore(*sets[n], *meshes[n])) for n in meshes}


@pytest.mark.parametrize('name', ['box', 'sphere', 'sphere4', 'torus', 'plate'])
def test_the_two_oracles_agree(name, scenes):
    s = scenes[name]
    c, (tm, _) = s['cast'], s['mt']
    ok = c['margin'] >= R.MARGIN
    hit = np.isfinite(c['t'])
    assert 0.05 * len(hit) < hit.sum() < 0.95 * len(hit)          # the set has hits and misses
    assert np.array_equal(np.isfinite(tm)[ok], hit[ok])
    both = ok & hit
    rel = np.abs(c['t'][both] - tm[both]) / np.abs(tm[both])
    print('%s: %d rays, %d hits, %d below the margin, max |t - t_MT| / |t| = %.3e'
          % (name, len(hit), hit.sum(), (~ok).sum(), rel.max()))
    assert rel.max() <= 1e-12
    # the fact the GPU tests lean on: at most 1 % of the rays are left out for margin
    assert (~ok).sum() <= 0.01 * len(ok)


def test_axis_rays_against_the_box():
    V, F = dict(R.shapes())['box']
    # z = -0.5 is faces 8 = (0, 2, 6) and 9 = (0, 6, 4); their shared diagonal runs from (-.5, -.5) to (.5, .5)
    assert np.array_equal(F[8], [0, 2, 6]) and np.array_equal(F[9], [0, 6, 4]) and (V[[0, 2, 6, 4], 2] == -0.5).all()
    xy = np.array([[0.1, 0.3], [0.3, 0.1], [0.25, 0.25], [-0.125, -0.125], [0.5, 0.1], [0.1, -0.5], [0.5, 0.5],
                   [-0.5, 0.5], [0.6, 0.0]])
    org = np.concatenate([xy, np.full((len(xy), 1), -2.0)], 1)
    d = np.tile([0.0, 0.0, 1.0], (len(xy), 1))
    c = R.cast(org, d, V, F)
    assert (c['t'][:8] == 1.5).all() and np.isinf(c['t'][8])      # interior, diagonal, edge, corner: no leak; outside
    assert c['face'][:4].tolist() == [8, 9, 8, 8]                 # on the diagonal: the lower of the two
    assert c['face'][8] == -1
    assert c['pair_hit'][2, 8] and c['pair_hit'][2, 9] and c['pair_t'][2, 8] == c['pair_t'][2, 9]
    # a direction twice as long halves t; from inside the far face is hit; backwards nothing with tmin = 0
    assert R.cast(org[:1], 2 * d[:1], V, F)['t'][0] == 0.75
    assert R.cast([[0.1, 0.2, 0.0]], [[0.0, 0.0, 1.0]], V, F)['t'][0] == 0.5
    assert np.isinf(R.cast(org[:1], -d[:1], V, F)['t'][0])
    assert R.cast(org[:1], -d[:1], V, F, tmin=-np.inf, tmax=0.0)['t'][0] == -2.5     # the lowest t in the window
    # a ray that starts on the surface: t = 0 counts with tmin = 0, the far side with tmin > 0; a hit exactly at tmax
    on = [[0.1, 0.2, -0.5]]
    assert R.cast(on, d[:1], V, F)['t'][0] == 0.0 and R.cast(on, d[:1], V, F, tmin=1e-3)['t'][0] == 1.0
    assert R.cast(org[:1], d[:1], V, F, tmax=1.5)['t'][0] == 1.5
    assert np.isinf(R.cast(org[:1], d[:1], V, F, tmax=np.nextafter(np.float32(1.5), np.float32(0)))['t'][0])
    # the cosine: -1 from outside (against the outward normal), +1 from inside
    assert c['cos'][0] == -1.0 and R.cast([[0.1, 0.2, 0.0]], [[0.0, 0.0, 1.0]], V, F)['cos'][0] == 1.0


def test_rays_through_the_centre_of_an_icosphere():
    V, F = dict(R.shapes())['sphere']
    centre, radius = np.array([0.07, -0.05, 0.03]), 0.55
    n = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    inradius = np.abs(np.einsum('ik,ik->i', n / np.linalg.norm(n, axis=1, keepdims=True), V[F[:, 0]] - centre)).min()
    assert 0.9 * radius < inradius < radius
    rng = np.random.default_rng(5)
    u = rng.normal(size=(500, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    org = R._f32(centre + 3.0 * u)
    d = R._f32(centre) - org                                   # aimed exactly at the centre, length about 3
    c = R.cast(org, d, V, F)
    assert np.isfinite(c['t']).all()
    r_hit = np.linalg.norm(c['point'] - centre, axis=1)
    assert (r_hit <= radius + 1e-6).all() and (r_hit >= inradius - 1e-6).all()
    assert (c['cos'] < 0).all()
    inside = R.cast(np.tile(R._f32(centre), (500, 1)), u, V, F)
    r_in = np.linalg.norm(inside['point'] - centre, axis=1)
    assert (r_in <= radius + 1e-6).all() and (r_in >= inradius - 1e-6).all() and (inside['cos'] > 0).all()


@pytest.mark.parametrize('name', R.CLOSED)
def test_no_miss_from_inside_a_closed_mesh(name):
    V, F = dict(R.shapes())[name]
    org, d = R.interior_rays(name, V, F)
    assert len(org) == len(V) + len(R.edges(F)) + 4096
    c = R.cast(org, d, V, F)
    assert (c['face'] >= 0).all() and (c['t'] > 0).all()


def test_rejects_and_degenerate_faces():
    V, F = dict(R.shapes())['box']
    org = np.array([[0.1, 0.2, -2.0]] * 5)
    d = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [np.nan, 0.0, 1.0], [0.0, np.inf, 1.0], [0.0, 0.0, 1.0]])
    org[4, 0] = np.nan
    c = R.cast(org, d, V, F)
    assert c['t'][0] == 1.5 and np.isinf(c['t'][1:]).all() and (c['face'][1:] == -1).all()
    assert np.isnan(c['point'][1:]).all() and np.isnan(c['cos'][1:]).all()
    # a zero-area face and a face seen edge-on never hit; a doubled face returns the lower index
    V2 = np.concatenate([V, [[0.1, 0.2, -1.0], [0.1, 0.2, -0.9], [0.1, 0.2, -0.8], [0.1, 0.9, -1.0]]])
    F2 = np.concatenate([[[8, 9, 10], [8, 9, 11]], F, F])
    c = R.cast(org[:1], d[:1], V2, F2)
    assert c['t'][0] == 1.5 and c['face'][0] == 2 + 8 and c['pair_hit'][0].sum() == 4      # near and far face, each doubled


def test_the_image_oracles_differ_only_near_edges():
    """Face ids of the rasteriser's oracle (screen coordinates snapped to 1/256 pixel) against the ray oracle on the
    same scene -- the 320-face sphere from the 20 FID views at 32 x 32: 8 of 20 480 pixels differ (3.9e-4), none of
    them in coverage.  tests/test_gpu_raycast.py allows the device twice that share."""
    V, F = dict(R.shapes())['sphere']
    share, cover = R.image_mismatch(V, F, 32)
    print('raster oracle against ray oracle: %d of %d pixels differ, %d in coverage' % (share, 20 * 32 * 32, cover))
    assert share == R.IMAGE_MISMATCH and cover == 0 and share <= 0.001 * 20 * 32 * 32
