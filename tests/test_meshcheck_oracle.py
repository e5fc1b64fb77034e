"""CPU checks that pin tests/meshcheck_oracle.py, the float64 restatement of the mesh checker's contract, to answers
written by hand (tests/meshcheck_cases.py): the planted pairs decide every branch of the pair rule on coordinates where
the arithmetic is exact; the cubes decide the counts; the general shapes give the figures the issue quotes.  No device.
"""
import numpy as np
import pytest

import meshcheck_cases as C
import meshcheck_oracle as MO

PAIRS = C.pairs()


@pytest.mark.parametrize('case', PAIRS, ids=[p[0] for p in PAIRS])
def test_planted_pair(case):
    name, v, f, hit, dup = case
    partners, first, pairs = MO.selfx(v, f)
    t = MO.topology(v, f)
    print(name, partners.tolist(), first.tolist(), pairs, t['duplicate_faces'])
    assert pairs == (1 if hit else 0)
    assert partners.tolist() == ([1, 1] if hit else [0, 0])
    assert first.tolist() == ([1, 0] if hit else [-1, -1])
    assert t['duplicate_faces'] == dup
    # the rule is one of the unordered pair: the faces swapped give the same answer
    assert MO.selfx(v, f[::-1])[2] == pairs
    # and it does not depend on which corner a face is stored from
    assert MO.selfx(v, np.roll(f, 1, axis=1))[2] == pairs


def test_edge_meets_is_closed_and_rejects_one_side():
    z = lambda *p: np.array([p], np.float64)
    a, b, c = z(0, 0, 0), z(4, 0, 0), z(0, 4, 0)
    assert MO.edge_meets(z(1, 1, -1), z(1, 1, 1), a, b, c)[0]
    assert MO.edge_meets(z(1, 1, 0), z(1, 1, 1), a, b, c)[0]           # an end point in the face
    assert MO.edge_meets(z(4, 0, 0), z(4, 0, 1), a, b, c)[0]           # on a vertex
    assert not MO.edge_meets(z(1, 1, 1), z(1, 1, 2), a, b, c)[0]       # both above
    assert not MO.edge_meets(z(3, 3, -1), z(3, 3, 1), a, b, c)[0]      # through the plane, outside
    assert not MO.edge_meets(z(5, 0, 0), z(8, 0, 0), a, b, c)[0]       # in the plane, collinear with an edge, apart
    assert MO.edge_meets(z(-1, 5, 0), z(5, -1, 0), a, b, c)[0]         # in the plane, along the hypotenuse


def test_det2_sign_is_exact():
    # 2^-30-sized products whose difference is below the rounding of either: the sign must still be the exact one
    e = 2.0 ** -30
    a = np.array([1 + e, 1 + e, 1.0])
    b = np.array([1 - e, 1 - e, 1.0])
    c = np.array([1.0, 1.0 - 2 ** -52, 1.0])
    d = np.array([1.0, 1.0, 1.0])
    assert MO._det2_sign(a, b, c, d).tolist() == [-1, 1, 0]


def test_weld_rule():
    nan = float('nan')
    v = np.array([[1, 2, 3], [0.0, 0, 0], [1, 2, 3], [-0.0, 0, -0.0], [nan, 0, 0], [nan, 0, 0], [1, 2, 3.0000002]],
                 np.float32)
    f = np.array([[0, 1, 2], [3, 2, 6]], np.int32)
    rep, nv, nf, index = MO.weld(v, f)
    assert rep.tolist() == [0, 1, 0, 1, 4, 5, 6]
    assert index.tolist() == [0, 1, 0, 1, 2, 3, 4]
    assert nv.shape == (5, 3) and nv[1].view(np.uint32).tolist() == [0, 0, 0]      # the representative's own bits
    assert nf.tolist() == [[0, 1, 0], [1, 0, 4]]                                    # a face that collapsed stays


def test_cube_soup_and_welded_cube():
    soup = C.unwelded(C.cube(2.0))
    assert soup[0].shape == (36, 3)
    t = MO.topology(*soup)
    assert t['components'] == 12 and t['edges'] == 36 and t['boundary_edges'] == 36
    # on the soup every neighbour touches: the reason check welds first
    assert MO.selfx(*soup)[2] > 0
    rep, v, f, index = MO.weld(*soup)
    assert len(v) == 8 and len(f) == 12
    t = MO.topology(v, f)
    d = MO.derived(t, len(f), len(v))
    assert t['edges'] == 18 and t['boundary_edges'] == 0 and t['nonmanifold_edges'] == 0
    assert t['inconsistent_edges'] == 0 and t['duplicate_faces'] == 0 and t['zero_area_faces'] == 0
    assert t['unreferenced_vertices'] == 0 and t['components'] == 1 and t['index_degenerate_faces'] == 0
    assert d['euler'] == 2 and d['genus'] == 0 and d['watertight'] and d['oriented'] and d['closed']
    assert abs(t['volume'] - 8.0) <= 1e-14 * t['volume_abs'] + 1e-14 and t['area'] == 24.0   # terms are n / 6
    assert (t['edge_faces'] == 2).all()
    partners, first, pairs = MO.selfx(v, f)
    assert pairs == 0 and not partners.any() and (first == -1).all()


def test_defective_cubes():
    _, v, f, _ = MO.weld(*C.two_cubes_sharing_an_edge())
    t = MO.topology(v, f)
    assert len(v) == 14 and t['nonmanifold_edges'] == 1 and t['boundary_edges'] == 0 and t['components'] == 1
    assert sorted(np.abs(t['edge_faces']).reshape(-1).tolist()).count(4) == 4
    assert not MO.derived(t, len(f), len(v))['watertight']
    t = MO.topology(*C.cube_one_face_flipped())
    assert t['inconsistent_edges'] == 3 and t['boundary_edges'] == 0
    assert (t['edge_faces'] == -2).sum() == 6
    d = MO.derived(t, 12, 8)
    assert d['watertight'] and not d['oriented'] and d['genus'] is None
    t = MO.topology(*C.cube_one_face_removed())
    assert t['boundary_edges'] == 3 and t['edges'] == 18 and (t['edge_faces'] == 1).sum() == 3
    assert not MO.derived(t, 11, 8)['closed']


def test_degenerate_and_unreferenced():
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [9, 9, 9], [1, 1, 0], [2, 2, 0]], np.float32)
    f = np.array([[0, 1, 2], [0, 1, 1], [0, 4, 5]], np.int32)
    t = MO.topology(v, f)
    assert t['index_degenerate_faces'] == 1 and t['zero_area_faces'] == 1
    assert t['unreferenced_vertices'] == 1 and t['edges'] == 6
    assert t['edge_faces'].tolist() == [[1, 1, 1], [0, 0, 0], [1, 1, 1]]
    assert t['area'] == 8.0


@pytest.fixture(scope='module')
def general():
    return dict(C.general())


@pytest.mark.parametrize('name, want', [('sphere', 0), ('torus', 0), ('open', 0), ('soup', 229)])
def test_winding_shapes(general, name, want):
    v, f = general[name]
    partners, first, pairs = MO.selfx(v, f)
    t = MO.topology(v, f)
    print(name, len(f), pairs, {k: t[k] for k in MO.K_COUNTS})
    assert pairs == want
    assert partners.sum() == 2 * pairs
    if name in ('sphere', 'torus'):
        d = MO.derived(t, len(f), len(v))
        assert d['watertight'] and d['oriented'] and d['genus'] == (0 if name == 'sphere' else 1)
    if name == 'open':
        assert t['boundary_edges'] > 0


def test_random_signs_mesh(general):
    v, f = general['random_signs']
    t = MO.topology(v, f)
    partners, first, pairs = MO.selfx(v, f)
    print('random_signs(12):', len(f), 'faces,', pairs, 'pairs,', {k: t[k] for k in MO.K_COUNTS})
    assert len(f) == 3340 and t['nonmanifold_edges'] == 6
    assert partners.sum() == 2 * pairs


def test_simplified_torus(general):
    v, f = general['simplified_torus']
    t = MO.topology(v, f)
    pairs = MO.selfx(v, f)[2]
    print('simplified torus:', len(f), 'faces,', pairs, 'pairs,', {k: t[k] for k in MO.K_COUNTS})
    assert t['nonmanifold_edges'] == 8
