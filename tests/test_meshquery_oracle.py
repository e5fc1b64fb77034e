"""CPU checks of the float64 point -> mesh oracle (tests/meshquery_oracle.py) itself, and of the query sets the GPU
tests use: the facts test_gpu_mesh_query.py relies on are established here, without a GPU."""
import numpy as np
import pytest

import mesh2sdf_oracle as O
import meshquery_oracle as Q


@pytest.fixture(scope='module')
def cases():
    meshes = Q.shapes()
    sets = Q.query_sets([m for _, m in meshes])
    return {name: (m, P) + Q.query(P, *m) for (name, m), P in zip(meshes, sets)}


def barycentric(p, a, b, c):
    """Least-squares weights of p in the plane of (a, b, c), and the residual off that plane."""
    w = np.empty((len(p), 3))
    res = np.empty(len(p))
    for i in range(len(p)):
        A = np.stack([a[i], b[i], c[i]], 1)
        A = np.concatenate([A, np.ones((1, 3))])
        x = np.linalg.lstsq(A, np.concatenate([p[i], [1.0]]), rcond=None)[0]
        w[i] = x
        res[i] = np.abs(A @ x - np.concatenate([p[i], [1.0]])).max()
    return w, res


@pytest.mark.parametrize('name', ['sphere', 'torus', 'box', 'plate'])
def test_closest_point_lies_on_its_face_at_the_distance(name, cases):
    (V, F), P, d, face, point = cases[name]
    assert len(P) == 4096 and len(F) == {'sphere': 320, 'torus': 256, 'box': 12, 'plate': 2}[name]
    assert np.array_equal(P, P.astype(np.float32).astype(np.float64))
    assert np.abs(np.linalg.norm(P - point, axis=1) - d).max() <= 1e-15
    t = F[face].astype(np.int64)
    w, res = barycentric(point, V[t[:, 0]], V[t[:, 1]], V[t[:, 2]])
    assert res.max() <= 1e-12                       # in the plane of its face
    assert w.min() >= -1e-12 and np.abs(w.sum(1) - 1).max() <= 1e-12
    # to_face on the winning face gives the winner back; all_faces has it as the row minimum
    d1, p1 = Q.to_face(P, V, F, face)
    assert np.array_equal(d1, d) and np.array_equal(p1, point)
    assert np.array_equal(Q.all_faces(P[:256], V, F).min(1), d[:256])


@pytest.mark.parametrize('name', ['sphere', 'torus', 'box', 'plate'])
def test_agrees_with_the_lattice_oracle(name, cases):
    (V, F), P, d, _, _ = cases[name]
    assert np.abs(d - O.udf(P, V, F)).max() <= 1e-14


def test_the_query_sets_are_what_the_gpu_tests_assume(cases):
    inside = {}
    for name in ('sphere', 'torus', 'box', 'plate'):
        (V, F), P, d, _, _ = cases[name]
        assert d.min() >= 1e-5, name                # no query is left out of a sign check
        if name != 'plate':
            w = O.winding(P, V, F)
            # integers to rounding: 6.7e-16, 7.9e-16 and 1.3e-15 (sphere, torus, box), so round() is beyond doubt
            assert np.abs(w - np.rint(w)).max() <= 2e-15, name
            inside[name] = int(Q.inside(P, V, F).sum())
    assert inside == {'sphere': 578, 'torus': 464, 'box': 346}


def test_unit_cube_regions():
    V, F = O.box(0.0, 1.0)
    P = np.array([[0.5, 0.25, 1.75],                 # above the face z = 1
                  [0.5, 0.5, 0.25],                  # inside: the nearest face is z = 0
                  [1.5, 2.0, 0.5],                   # off the edge x = 1, y = 1
                  [-0.25, 0.5, -0.5],                # off the edge x = 0, z = 0
                  [1.5, 1.25, 2.0],                  # off the vertex (1, 1, 1)
                  [-1.0, -2.0, -2.0],                # off the vertex (0, 0, 0)
                  [0.25, 0.75, 1.0]])                # on the surface
    want_d = [0.75, 0.25, np.hypot(0.5, 1.0), np.hypot(0.25, 0.5), np.sqrt(0.25 + 0.0625 + 1.0), 3.0, 0.0]
    want_p = [[0.5, 0.25, 1.0], [0.5, 0.5, 0.0], [1.0, 1.0, 0.5], [0.0, 0.5, 0.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0],
              [0.25, 0.75, 1.0]]
    d, face, point = Q.query(P, V, F)
    assert np.abs(d - want_d).max() <= 1e-15
    assert np.abs(point - want_p).max() <= 1e-15
    assert Q.inside(P[:6], V, F).tolist() == [False, True, False, False, False, False]


def test_zero_area_triangles_are_their_edges():
    V = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.5, 0.5, 0.5]])
    F = np.array([[0, 1, 2], [3, 3, 3], [0, 2, 2]], np.int32)           # a collinear triangle, a point, a segment
    P = np.array([[1.5, 1.0, 0.0], [3.0, 0.0, 4.0], [0.5, 0.5, 0.75]])
    d, face, point = Q.query(P, V, F)
    assert np.allclose(d, [1.0, np.hypot(1.0, 4.0), 0.25], atol=1e-15)
    assert face.tolist() == [0, 0, 1]
    assert np.allclose(point, [[1.5, 0, 0], [2, 0, 0], [0.5, 0.5, 0.5]], atol=1e-15)
    assert np.isfinite(Q.all_faces(P, V, F)).all()
