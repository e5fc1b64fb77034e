"""CPU checks that pin tests/normals_oracle.py -- the numpy restatement the GPU tests of octfusion_amd.normals compare
against -- to shapes whose normals are known: points uniform by area on a sphere, a torus, two spheres, a box and a thin
plate, k = 16, S = 8, rounds = 3, the automatic grid.

Smooth shapes must come out with no wrong and no undecided sign.  On the box and the plate the PCA normal of a point
next to an edge is a mixture of two faces (unoriented error up to 87 degrees), so there only points whose unoriented
error is below 45 degrees must carry the right sign.  The unoriented error of the smooth shapes has no preset bound:
ANGLE holds the maximum measured on this oracle for the committed seed, and the test asserts 1.5 x that -- the bound
guards against a broken covariance (which gives tens of degrees), not against sampling luck."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import normals_oracle as O

# name -> (sampler, automatic G seen, measured maximum unoriented angle in degrees or None)
CASES = {
    'sphere_500': (lambda: O.sphere(500), 8, 7.265),
    'sphere_2000': (lambda: O.sphere(2000), 11, 5.253),
    'torus_2000': (lambda: O.torus(2000), 14, 14.619),
    'torus_4000': (lambda: O.torus(4000), 21, 10.097),
    'two_spheres': (lambda: O.two_spheres(2000), 31, 6.570),
    'box': (lambda: O.box(6000), 23, None),
    'plate': (lambda: O.plate(6000), 27, None),
}


@functools.lru_cache(maxsize=None)
def run(name):
    p, n = CASES[name][0]()
    out, un, s, G, counts = O.estimate(p, k=16, steps=8, rounds=3)
    return p, n, out, un, s, G, counts


@pytest.mark.parametrize('name', ['sphere_500', 'sphere_2000', 'torus_2000', 'torus_4000', 'two_spheres'])
def test_smooth_shapes_are_oriented_outward(name):
    p, n, out, un, s, G, counts = run(name)
    assert G == CASES[name][1]
    assert counts['undecided'] == 0 and counts['degenerate'] == 0
    assert int(((out.astype(np.float64) * n).sum(1) < 0).sum()) == 0
    assert np.array_equal(out, np.where((s == -1)[:, None], -un, un))
    ang = O.angle_deg(un, n).max()
    print(name, 'max unoriented angle', ang)
    assert ang <= 1.5 * CASES[name][2]            # measured: the third entry of CASES
    assert np.abs(np.linalg.norm(out.astype(np.float64), axis=1) - 1).max() <= 1e-6


@pytest.mark.parametrize('name', ['box', 'plate'])
def test_flat_shapes_are_oriented_where_the_normal_is_defined(name):
    p, n, out, un, s, G, counts = run(name)
    assert G == CASES[name][1]
    assert counts['undecided'] == 0 and counts['degenerate'] == 0
    good = O.angle_deg(un, n) < 45.0
    assert good.mean() > 0.9
    assert int((((out.astype(np.float64) * n).sum(1) < 0) & good).sum()) == 0


def test_fma32_is_one_rounding():
    """Against exact rational arithmetic, with addends from 2^-60 to 2^8 times the product: the float64 sum is
    inexact for most of them, and a small addend decides which way a product near a float32 boundary rounds."""
    rng = np.random.default_rng(5)
    a = rng.uniform(0.5, 2.0, 400).astype(np.float32)
    b = a.copy()
    c = (rng.uniform(0.5, 2.0, 400) * 2.0 ** rng.integers(-60, 8, 400)).astype(np.float32)
    got = O.fma32(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo = np.float32(float(exact))             # float(Fraction) rounds correctly to float64, then to float32 ...
        cands = {np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))}
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(v.view(np.uint32)) & 1))
        assert g == best                          # ... so pick the nearest of the three neighbours exactly


def test_knn_order_and_padding():
    p = O.lattice(300, seed=2)
    idx, d2 = O.knn(p, 33)
    assert (idx[:, 0] == np.arange(300)).all() and (d2[:, 0] == 0).all()
    assert (np.diff(d2.astype(np.float64), axis=1) >= 0).all()
    tie = np.diff(d2, axis=1) == 0
    assert tie.sum() > 1000 and (np.diff(idx, axis=1)[tie] > 0).all()       # equal distance: ascending index
    q = np.concatenate([p[:4], p[:1]])                                      # point 4 duplicates point 0
    idx, d2 = O.knn(q, 16)
    assert idx[4, 0] == 0 and idx[4, 1] == 4 and (d2[4, :2] == 0).all()
    assert (idx[:, 5:] == -1).all() and np.isinf(d2[:, 5:]).all()


def test_pca_degenerate_and_sign():
    p = np.concatenate([np.zeros((6, 3)), np.arange(6)[:, None] * [[1.0, 2.0, 0.5]]]).astype(np.float32)
    ident = np.tile(np.arange(6), (6, 1))
    nrm, var, deg, _ = O.pca(p[:6], ident)                    # identical points: a zero covariance
    assert deg.all() and (nrm == 0).all() and (var == 0).all()
    few = np.full((6, 6), -1)
    few[:, :2] = ident[:, :2]
    assert O.pca(p[6:], few)[2].all()                         # two neighbours
    nrm, var, deg, gap = O.pca(p[6:], ident)                  # collinear: a unit normal across the line, variation ~ 0
    assert not deg.any() and np.abs(nrm.astype(np.float64) @ [1.0, 2.0, 0.5]).max() < 1e-6 and var.max() < 1e-12
    pp, nn = O.sphere(400, seed=3)
    nrm, _, deg, _ = O.pca(pp, O.knn(pp, 12)[0])
    lead = np.abs(nrm).argmax(1)
    assert not deg.any() and (nrm[np.arange(400), lead] > 0).all()
