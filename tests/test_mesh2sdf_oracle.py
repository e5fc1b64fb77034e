"""The float64 oracle of the mesh -> SDF lattice (tests/mesh2sdf_oracle.py) against facts that need no oracle: rigorous
bounds on the distance to an icosphere, the winding number being an integer off the surface, exact counts on a box
whose faces lie on lattice planes, and zero-area triangles against their segments."""
import numpy as np
import pytest

import mesh2sdf_oracle as O

C = np.array([0.07, -0.05, 0.03])
R = 0.55


@pytest.fixture(scope='module')
def sphere():
    V, F = O.icosphere(2, C, R)
    P = O.lattice(16)
    return V, F, P, O.udf(P, V, F)


def test_makers():
    V, F = O.icosphere(2, C, R)
    assert F.shape == (320, 3) and V.shape == (162, 3)
    assert O.icosphere(4)[1].shape == (5120, 3)
    V, F = O.torus(16, 8, 0.5, 0.2)
    assert F.shape == (256, 3) and V.shape == (128, 3)
    assert O.box()[1].shape == (12, 3) and O.plate()[1].shape == (2, 3)
    for v, _ in (O.icosphere(1), O.torus(), O.box(-0.3, 0.7), O.plate()):
        assert np.array_equal(v, v.astype(np.float32).astype(np.float64))        # rounded through fp32


def test_sphere_bounds(sphere):
    V, F, P, d = sphere
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    r_in = np.abs(((a - C) * n).sum(1)).min()            # the smallest centre-to-face-plane distance
    r_out = np.linalg.norm(V - C, axis=1).max()          # fp32 rounding moves a vertex off the sphere by ~1e-8
    assert 0.9 * R < r_in < R and abs(r_out - R) < 1e-7
    q = np.linalg.norm(P - C, axis=1)
    out, inn = q >= r_out, q <= r_in
    assert out.sum() > 2000 and inn.sum() > 100
    # the mesh lies between the spheres r_in and r_out
    assert (d[out] >= q[out] - r_out - 1e-12).all() and (d[out] <= q[out] - r_in + 1e-12).all()
    assert (d[inn] >= r_in - q[inn] - 1e-12).all() and (d[inn] <= r_out - q[inn] + 1e-12).all()


def test_winding_is_an_integer(sphere):
    V, F, P, d = sphere
    for (v, f), dist in (((V, F), d), (O.torus(16, 8, 0.5, 0.2, (0.03, 0.02, -0.04)), None)):
        dist = O.udf(P, v, f) if dist is None else dist
        w = O.winding(P, v, f)
        off = dist > 1e-5
        err = np.abs(w - np.rint(w))[off].max()
        print('winding: max distance from an integer %.2e' % err)
        assert err < 1e-12
        assert set(np.unique(np.abs(np.rint(w[off])))) == {0.0, 1.0}


def test_aligned_box_counts():
    V, F = O.box(-0.5, 0.5)
    P = O.lattice(16)
    s, d = O.sdf(P, V, F)
    assert int((d == 0).sum()) == 9 ** 3 - 7 ** 3 == 386
    assert int(((s < 0) & (d > 0)).sum()) == 343
    i = np.rint((P + 1) * 8).astype(int)
    strictly = ((i > 4) & (i < 12)).all(1)
    assert np.array_equal(strictly, (s < 0) & (d > 0))
    out = ~(((i >= 4) & (i <= 12)).all(1))
    ref = np.linalg.norm(np.maximum(np.abs(P) - 0.5, 0.0), axis=1)
    assert np.abs(d[out] - ref[out]).max() < 1e-15


def test_zero_area_triangles():
    """A repeated vertex, a collinear triple and a point are the segment or point they are."""
    V = O._f32([[0.1, 0.2, 0.3], [0.4, -0.1, 0.2], [0.25, 0.05, 0.25], [0.7, -0.4, 0.1]])
    P = O.lattice(8)
    seg = np.sqrt(O._segment2(P, V[0], V[1]))
    assert np.allclose(O.udf(P, V, [[0, 0, 1]]), seg, rtol=0, atol=1e-15)
    assert np.allclose(O.udf(P, V, [[0, 1, 1]]), seg, rtol=0, atol=1e-15)
    W = np.array([[-0.25, 0.125, 0.5], [0.0, 0.25, 0.25], [0.5, 0.5, -0.25]])       # exactly collinear, middle first
    assert (np.cross(W[1] - W[0], W[2] - W[0]) == 0).all()
    assert np.allclose(O.udf(P, W, [[1, 0, 2]]), np.sqrt(O._segment2(P, W[0], W[2])), rtol=0, atol=1e-15)
    assert np.allclose(O.udf(P, V, [[3, 3, 3]]), np.linalg.norm(P - V[3], axis=1), rtol=0, atol=1e-15)
    assert np.isfinite(O.udf(P, V, [[0, 0, 1], [3, 3, 3], [0, 1, 2]])).all()
