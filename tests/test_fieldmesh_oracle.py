"""CPU checks of tests/fieldmesh_oracle.py, the numpy restatement of the field-meshing contract
(csrc/ofx_fieldmesh.hip), against tests/mc_oracle.py on hand-made node sets."""
import numpy as np
import pytest

import fieldmesh_oracle as F
import mc_oracle as M

DE = 5                                            # 32^3 finest cells


def _shell_nodes(r=0.5, width=1):
    """Depth-DE cells within `width` cells of the sphere |x| = r."""
    S = 1 << DE
    c = (np.arange(S) + 0.5) * (2.0 / S) - 1.0
    x, y, z = np.meshgrid(c, c, c, indexing='ij')
    d = np.abs(np.sqrt(x * x + y * y + z * z) - r)
    return np.argwhere(d <= width * 2.0 / S)


def _random_nodes(seed, n=40):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << DE, (n, 3))


FIELDS = {
    'sphere': lambda R: M.sphere(R),
    'gaussians': lambda R: M.gaussians(R),
    'random_signs': lambda R: M.random_signs(R, seed=3),
}
NODES = {'shell': _shell_nodes(), 'random': _random_nodes(1), 'one': np.array([[3, 17, 30]])}


def _leaks_brute_force(sdf, level, act):
    """Distinct crossing edges inside a face shared by an active and an inactive brick."""
    R = sdf.shape[0]
    nb = act.shape[0]
    inside = sdf < np.float32(level)
    found = set()
    for I in np.ndindex(nb, nb, nb):
        for c in range(3):
            J = list(I)
            J[c] += 1
            if J[c] >= nb or act[I] == act[tuple(J)]:
                continue
            lo = [8 * i for i in I]
            hi = [min(8 * i + 8, R - 1) for i in I]
            lo[c] = hi[c] = 8 * J[c]                    # the shared plane
            for a in range(3):
                if a == c:
                    continue
                for x in range(lo[0], hi[0] + 1):
                    for y in range(lo[1], hi[1] + 1):
                        for z in range(lo[2], hi[2] + 1):
                            q = [x, y, z]
                            q[a] += 1
                            if q[a] > hi[a]:
                                continue
                            if inside[x, y, z] != inside[tuple(q)]:
                                found.add((x, y, z, a))
    return len(found)


@pytest.mark.parametrize('field', sorted(FIELDS))
@pytest.mark.parametrize('R', [9, 20, 33])
def test_all_active_equals_dense(field, R):
    sdf = FIELDS[field](R)
    level = 0.0 if field != 'gaussians' else 0.01
    dv, df = M.marching_cubes(sdf, level)
    v, f, st = F.field_mesh(sdf, DE, NODES['one'], margin=1 << DE, level=level)
    nb = F.n_bricks(R)
    assert st['bricks'] == nb ** 3 and st['leaks'] == 0 and st['active'].all()
    assert np.array_equal(F.canonical_triangles(v, f), F.canonical_triangles(dv, df))
    assert len(v) == len(dv)
    assert np.array_equal(v[np.lexsort(v.T)].view(np.uint32), dv[np.lexsort(dv.T)].view(np.uint32))
    if nb == 1:                                       # one brick: the order is the dense order too
        assert np.array_equal(v.view(np.uint32), dv.view(np.uint32)) and np.array_equal(f, df)
    # a dense depth (nodes=None) activates everything as well
    v2, f2, st2 = F.field_mesh(sdf, DE, None, margin=0, level=level)
    assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and np.array_equal(f2, f)
    assert st2['seeds'] == nb ** 3


@pytest.mark.parametrize('nodes', sorted(NODES))
@pytest.mark.parametrize('R', [17, 33, 40])
def test_active_set_grows_with_margin(nodes, R):
    prev = None
    for m in (0, 1, 2, 3, 8, 1 << DE):
        act = F.active_bricks(R, DE, NODES[nodes], m)
        if prev is not None:
            assert (act | ~prev).all(), 'a brick active at a smaller margin is inactive at margin %d' % m
        prev = act
    assert prev.all()
    assert not F.active_bricks(R, DE, np.zeros((0, 3), np.int64), 5).any()


@pytest.mark.parametrize('field', sorted(FIELDS))
@pytest.mark.parametrize('nodes', sorted(NODES))
@pytest.mark.parametrize('m', [0, 1])
def test_restriction_and_leaks(field, nodes, m):
    R = 33
    sdf = FIELDS[field](R)
    dv, df = M.marching_cubes(sdf, 0.0)
    v, f, st = F.field_mesh(sdf, DE, NODES[nodes], margin=m, level=0.0)
    act = st['active']
    assert st['bricks'] == int(act.sum()) and st['seeds'] <= st['bricks']
    # every kept triangle's cell is active, and exactly the triangles of active cells are kept
    cells = F.dense_cells_of_faces(sdf, 0.0)
    keep = act[cells[:, 0] // 8, cells[:, 1] // 8, cells[:, 2] // 8]
    assert len(f) == int(keep.sum())
    assert np.array_equal(F.canonical_triangles(v, f), F.canonical_triangles(dv, df[keep]))
    # every vertex is referenced
    if len(f):
        assert np.array_equal(np.unique(f), np.arange(len(v)))
    else:
        assert len(v) == 0
    assert st['leaks'] == _leaks_brute_force(sdf, 0.0, act)


def test_sphere_shell_band_is_leak_free():
    """The node set that follows the surface: the band holds the whole surface, so nothing leaks and the restricted
    mesh is the dense one, while some bricks stay inactive."""
    R = 65
    sdf = M.sphere(R)
    dv, df = M.marching_cubes(sdf, 0.0)
    v, f, st = F.field_mesh(sdf, DE, NODES['shell'], margin=1, level=0.0)
    assert st['leaks'] == 0 and st['bricks'] < F.n_bricks(R) ** 3
    assert np.array_equal(F.canonical_triangles(v, f), F.canonical_triangles(dv, df))
    assert M.directed_edge_balance(f) and M.euler(v, f) == 2
