"""CPU pins of tests/smooth_oracle.py (the float64 restatement of csrc/ofx_meshsmooth.hip's contract) to answers worked
out by hand, plus the host-side pieces of the feature: ``write_obj(normals=)`` and the command-line parsers.
tests/test_gpu_mesh_smooth.py holds the device to the oracle."""
import numpy as np

import meshcheck_cases as C
import smooth_oracle as SO
from smooth_cases import TETRA, fan



def rows(adj, what='nbr', off='row_off'):
    return [adj[what][adj[off][i]:adj[off][i + 1]].tolist() for i in range(len(adj[off]) - 1)]


# ---- pin 1: rows, flags and corner lists ----------------------------------------------------------------------------
def test_adjacency_of_the_tetrahedron_and_the_cube():
    t = SO.adjacency(*TETRA)
    assert rows(t) == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]
    assert t['vflags'].tolist() == [1, 1, 1, 1]
    assert rows(t, 'corner', 'corner_off') == [[0, 3, 9], [2, 4, 6], [1, 7, 11], [5, 8, 10]]
    c = SO.adjacency(*C.cube(2.0))
    assert rows(c) == [[1, 2, 3, 4, 5, 6], [0, 3, 5, 7], [0, 3, 6, 7], [0, 1, 2, 7], [0, 5, 6, 7], [0, 1, 4, 7],
                       [0, 2, 4, 7], [1, 2, 3, 4, 5, 6]]
    assert c['row_off'].tolist() == [0, 6, 10, 14, 18, 22, 26, 30, 36] and c['vflags'].tolist() == [1] * 8
    cr = rows(c, 'corner', 'corner_off')
    assert cr[0] == [0, 3, 12, 15, 24, 27] and cr[1] == [5, 13, 30, 33] and cr[7] == [8, 10, 19, 23, 32, 34]
    assert c['corner_off'].tolist() == [0, 6, 10, 14, 18, 22, 26, 30, 36]
    assert sorted(c['corner'].tolist()) == list(range(36))


def test_flags_of_boundary_and_nonmanifold_vertices_and_faces_that_take_no_part():
    hole = SO.adjacency(*C.cube_one_face_removed())
    assert hole['vflags'].tolist() == [1, 1, 3, 1, 1, 1, 3, 3]          # the hole's vertices 2, 6, 7
    book = SO.adjacency(np.zeros((5, 3), np.float32), [[0, 1, 2], [0, 1, 3], [0, 1, 4]])
    assert book['vflags'].tolist() == [7, 7, 3, 3, 3]                   # three faces on the edge 0 - 1
    v, f = C.cube(2.0)
    more = SO.adjacency(np.concatenate([v, [[np.nan] * 3, [9, 9, 9]]]).astype(np.float32),
                        np.concatenate([[[3, 3, 1]], f, [[0, 9, 9]]]))
    assert rows(more)[:8] == rows(SO.adjacency(v, f)) and rows(more)[8:] == [[], []]
    assert more['vflags'].tolist() == [1] * 8 + [0, 0]
    assert rows(more, 'corner', 'corner_off')[0] == [3, 6, 15, 18, 27, 30]          # every face one further on
    assert not SO.refused(np.concatenate([v, [[np.nan] * 3]]).astype(np.float32), f)
    assert SO.refused(v, [[0, 1, 8]]) and SO.refused(np.where(np.arange(8)[:, None] == 5, np.nan, v), f)


# ---- pin 2: vertex normals of the cube ------------------------------------------------------------------------------
def test_angle_weighted_normals_of_the_cube_are_its_diagonals_exactly():
    v, f = C.cube(2.0)
    want = (v.astype(np.float64) - 1.0) / np.sqrt(3.0)
    n, s, lengths = SO.vertex_normals(v, f, SO.ANGLE)
    assert np.abs(n - want).max() == 0.0
    assert np.abs(s).max() == np.pi / 2 and (lengths >= np.pi / 2).all()
    # the other two weights follow the triangulation: a corner with two faces on a side leans towards it
    for mode in (SO.AREA, SO.UNIFORM):
        dev = np.abs(SO.vertex_normals(v, f, mode)[0] - want).max()
        assert 0.2 < dev < 0.3, dev
        print('mode %d: off the diagonal by %.3f' % (mode, dev))


def test_a_face_without_area_and_an_unused_vertex_add_nothing():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [5, 5, 5]], np.float32)
    n, _, _ = SO.vertex_normals(v, [[0, 1, 2], [0, 1, 3]], SO.ANGLE)       # the second face is a segment
    assert n.tolist() == [[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 0], [0, 0, 0]]


# ---- pins 3 and 4: the hexagon fan ----------------------------------------------------------------------------------
def test_one_laplacian_step_puts_the_centre_of_a_fan_on_the_centroid_of_its_rim():
    v, f = fan(6, (0.3, 0.2, 0.5))
    out = SO.smooth(v, f, iterations=1, lam=1.0, mu=None, weights=0, boundary=SO.FIXED)
    rim = v[1:].astype(np.float64)
    assert np.abs(out[0] - rim.mean(axis=0)).max() < 1e-15
    assert np.array_equal(out[1:], rim)                                 # the rim is the boundary: fixed
    assert np.array_equal(SO.smooth(v, f, iterations=0), v.astype(np.float64))


def test_cotangent_weights_of_a_flat_regular_fan_are_equal():
    v, f = fan(6, (0.0, 0.0, 0.0))
    uni = SO.smooth(v, f, iterations=1, lam=1.0, mu=None, weights=0)
    cot = SO.smooth(v, f, iterations=1, lam=1.0, mu=None, weights=1)
    assert np.abs(cot - uni).max() < 1e-15 and np.abs(cot[0]).max() < 1e-15
    v, f = fan(6, (0.3, 0.2, 0.0))                                      # off centre, still in the rim's plane
    cot = SO.smooth(v, f, iterations=1, lam=1.0, mu=None, weights=1)
    assert abs(cot[0, 2]) == 0.0 and np.array_equal(cot[1:], v[1:].astype(np.float64))


# ---- pins 5 and 6: the boundary rules -------------------------------------------------------------------------------
def test_slide_keeps_the_hole_in_its_plane_and_fixed_keeps_its_bits():
    v, f = C.cube_one_face_removed()
    hole = [2, 6, 7]
    assert (v[hole, 1] == 2.0).all()
    for weights in (0, 1):
        for mu in (None, -0.53):
            slide = SO.smooth(v, f, iterations=10, lam=0.5, mu=mu, weights=weights, boundary=SO.SLIDE)
            assert (slide[hole, 1] == 2.0).all()
            assert not np.array_equal(slide[hole], v[hole].astype(np.float64))          # and they do move along it
            fixed = SO.smooth(v, f, iterations=10, lam=0.5, mu=mu, weights=weights, boundary=SO.FIXED)
            assert np.array_equal(fixed[hole], v[hole].astype(np.float64))
            free = SO.smooth(v, f, iterations=10, lam=0.5, mu=mu, weights=weights, boundary=SO.FREE)
            assert (free[hole, 1] != 2.0).all()


def test_the_order_of_a_rows_terms_moves_the_result_by_rounding_only():
    rng = np.random.default_rng(0)
    v, f = fan(12, (0.1, 0.2, 0.7), rim_z=0.25)
    v = (v * (1 + 0.05 * rng.standard_normal(v.shape))).astype(np.float32)
    for weights in (0, 1):
        a = SO.smooth(v, f, 10, weights=weights, boundary=SO.FREE)
        b = SO.smooth(v, f, 10, weights=weights, boundary=SO.FREE, shuffle=rng)
        assert np.abs(a - b).max() < 1e-14


# ---- pin 7: OBJ files with normals ----------------------------------------------------------------------------------
def test_write_obj_with_normals_round_trips_and_without_is_unchanged(tmp_path):
    from octfusion_amd import mesh
    v, f = C.cube(2.0)
    v = (v + np.float32(0.1)).astype(np.float32)
    n = SO.vertex_normals(v, f, SO.ANGLE)[0].astype(np.float32)
    plain, kw, withn = (str(tmp_path / k) for k in ('plain.obj', 'kw.obj', 'n.obj'))
    assert mesh.write_obj(plain, v, f) and mesh.write_obj(kw, v, f, normals=None) and mesh.write_obj(withn, v, f, n)
    want = ''.join('v %.9g %.9g %.9g\n' % tuple(float(x) for x in row) for row in v)
    want += ''.join('f %d %d %d\n' % tuple(int(x) + 1 for x in row) for row in f)
    assert open(plain).read() == want == open(kw).read()
    rv, rf = mesh.read_obj(withn)
    assert np.array_equal(rv.view(np.uint32), v.view(np.uint32)) and np.array_equal(rf, f)
    lines = open(withn).read().splitlines()
    vn = np.array([l.split()[1:] for l in lines if l.startswith('vn ')], np.float64).astype(np.float32)
    assert np.array_equal(vn.view(np.uint32), n.view(np.uint32))
    assert [l for l in lines if l.startswith('f ')][0] == 'f 1//1 3//3 4//4'
    assert [l[:2] for l in lines] == ['v '] * 8 + ['vn'] * 8 + ['f '] * 12


# ---- pin 8: the command lines ---------------------------------------------------------------------------------------
def test_parsers_take_the_new_flags():
    from octfusion_amd import generate, mesh_smooth
    a = generate.parser().parse_args(['--mesh', '--smooth', '10', '--smooth-normals', '--check', '--out', 'x'])
    assert a.smooth == 10 and a.smooth_normals and a.mesh
    a = generate.parser().parse_args(['--mesh'])
    assert a.smooth is None and not a.smooth_normals
    a = mesh_smooth.parser().parse_args(['--input', 'a.obj', 'b.obj', '--out', 'd', '--iterations', '3', '--lambda',
                                         '0.4', '--mu', '-0.45', '--weights', 'cot', '--boundary', 'slide',
                                         '--normals'])
    assert (a.input, a.out, a.iterations, a.lam, a.mu, a.weights, a.boundary, a.normals, a.laplacian) == (
        ['a.obj', 'b.obj'], 'd', 3, 0.4, -0.45, 'cot', 'slide', 'angle', False)
    a = mesh_smooth.parser().parse_args(['--input', 'a.obj', '--out', 'd', '--laplacian', '--normals', 'area'])
    assert a.laplacian and a.normals == 'area' and a.iterations == 10 and a.lam == 0.5 and a.mu == -0.53


def test_the_new_entry_points_are_bound():
    from octfusion_amd import _lib
    for name in ('ofx_mesh_adjacency', 'ofx_mesh_vertex_normals', 'ofx_mesh_smooth'):
        assert name in _lib.EXPORTS and name + '_ws_bytes' in _lib.EXPORTS
