"""CPU checks of tests/winding_oracle.py: the conditions the GPU tests (tests/test_gpu_winding.py) lean on, with the
numbers printed (run with -s to see them; DESIGN.md 4.21 quotes the far-field errors)."""
import numpy as np
import pytest

import mesh2sdf_oracle as O
import meshquery_oracle as Q
import winding_oracle as W


@pytest.fixture(scope='module')
def cases():
    meshes = W.shapes()
    sets = W.query_sets([m for _, m in meshes])
    return {name: {'mesh': m, 'P': P, 'w': W.exact(P, *m)} for (name, m), P in zip(meshes, sets)}


def test_shapes_and_sets(cases):
    assert list(cases) == ['sphere', 'torus', 'open', 'soup', 'plate']
    assert [len(c['mesh'][1]) for c in cases.values()] == [1280, 1024, 1040, 2574, 2]
    assert [len(c['mesh'][1]) % 64 for c in cases.values()] == [0, 0, 16, 14, 2]      # whole and ragged staging rounds
    for c in cases.values():
        assert c['P'].shape == (W.N_QUERIES, 3) and np.array_equal(c['P'].astype(np.float32).astype(np.float64), c['P'])
        assert W.with_area(*c['mesh']).all()
    # the automatic grid never reaches the far field's interesting sizes here: tests pass bins
    assert [W.auto_bins(len(c['mesh'][1])) for c in cases.values()] == [3, 2, 3, 4, 1]
    assert W.auto_bins(256) == 1 and W.auto_bins(257) == 2 and W.auto_bins(10 ** 7) == 16 and W.auto_bins(99, 5) == 5


@pytest.mark.parametrize('name,count', [('sphere', 619), ('torus', 514)])
def test_closed_shapes_agree_with_the_parity_oracle(name, count, cases):
    c = cases[name]
    inside = c['w'] > 0.5
    assert np.array_equal(inside, O.inside(c['P'], *c['mesh'])) and int(inside.sum()) == count
    assert np.abs(c['w'] - np.rint(c['w'])).max() <= 1e-12


def test_ranges_and_borderline_queries(cases):
    near, band = [], []
    for name, c in cases.items():
        w = c['w']
        d = Q.query(c['P'], *c['mesh'])[0]
        near.append(int((d < 1e-5).sum()))
        band.append(int((np.abs(w - 0.5) < 0.06).sum()))
        print('%s: w in [%.4f, %.4f], %d inside, %d within 1e-5 of the mesh, %d with |w - 0.5| < 0.06'
              % (name, w.min(), w.max(), int((w > 0.5).sum()), near[-1], band[-1]))
    w = cases['open']['w']
    assert -0.2 < w.min() < -0.1 and 0.9 < w.max() < 1.0                 # a hole: neither 0 nor 1 is reached cleanly
    w = cases['soup']['w']
    assert w.min() < -0.2 and w.max() > 3.3                              # negative values and |w| > 1
    w = cases['plate']['w']
    assert -0.5 < w.min() < -0.49 and 0.49 < w.max() < 0.5
    assert max(near) <= 0.001 * W.N_QUERIES and max(band) <= 0.01 * W.N_QUERIES


def test_zero_area_faces_contribute_nothing(cases):
    c = cases['sphere']
    V, F = c['mesh']
    flat = np.array([[5, 5, 5], [3, 9, 3]], np.int32)
    assert W.with_area(V, flat).tolist() == [False, False]
    assert np.array_equal(W.exact(c['P'][:100], V, np.concatenate([flat, F])), c['w'][:100])
    assert (W.exact(c['P'][:100], V, flat) == 0).all()
    assert np.abs(W.exact(c['P'][:100], V, np.concatenate([F, F])) - 2 * c['w'][:100]).max() <= 1e-12


@pytest.mark.parametrize('bins,beta', W.FAR_SETTINGS)
def test_far_field_restatement(bins, beta, cases):
    for name in ('sphere', 'torus', 'open', 'soup'):
        c = cases[name]
        wf, margin, share = W.far(c['P'], *c['mesh'], bins, beta)
        E = np.abs(wf - c['w']).max()
        flips = int(((wf > 0.5) != (c['w'] > 0.5)).sum())
        left = int((np.abs(c['w'] - 0.5) <= 2 * E).sum())
        print('%s bins %d beta %g: E = %.3e, %d flips at 0.5, %d queries with |w - 0.5| <= 2 E, %.1f %% of the '
              '(query, bin) decisions far, smallest margin %.2e, %d margins <= 1e-9'
              % (name, bins, beta, E, flips, left, 100 * share, margin.min(), int((margin <= 1e-9).sum())))
        assert 2 * E <= 0.06                    # the band test_ranges_and_borderline_queries counts: <= 15 queries
        assert flips == 0
        assert left <= 0.01 * W.N_QUERIES and (margin <= 1e-9).sum() <= 0.001 * W.N_QUERIES
        assert share > 0.5                                              # the far field is in fact used
        if beta == 2.0:                         # a wider opening angle is a worse approximation
            assert E > np.abs(W.far(c['P'], *c['mesh'], bins, 3.0)[0] - c['w']).max()
    # all bins near: the exact value, up to the order of the sums
    c = cases['torus']
    wn, _, share = W.far(c['P'][:256], *c['mesh'], bins, 1.0e6)
    assert share == 0 and np.abs(wn - c['w'][:256]).max() <= 1e-12


def test_dipole_converges_with_the_cube_of_the_distance():
    """One patch (a bin of the sphere) seen from 200 directions at 32, 64, 128 and 256 radii: the dipole's largest error
    falls as d^-3 (the quadrupole term it leaves out), so doubling d divides it by about 8 (from
    above: the next term falls as d^-4)."""
    V, F = W.shapes()[0][1]
    _, N, centre, r, idx = W.moments(V, F, 4)[0]
    u = np.random.default_rng(1).normal(size=(200, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    errs = []
    for k in (32, 64, 128, 256):
        P = centre + k * r * u
        d = centre - P
        dipole = (d @ N) / (4 * np.pi * np.linalg.norm(d, axis=1) ** 3)
        errs.append(float(np.abs(dipole - O.winding(P, V, F[idx])).max()))
    ratios = [a / b for a, b in zip(errs, errs[1:])]
    print('largest dipole error at 32, 64, 128, 256 radii: %s; ratios %s' % (errs, ratios))
    assert all(8.0 < q < 9.5 for q in ratios) and ratios[0] > ratios[1] > ratios[2]
