"""The meshes of the mesh-checker tests with their hand-written answers (tests/test_meshcheck_oracle.py pins the oracle
to them on the CPU, tests/test_gpu_meshcheck.py runs the device on the same meshes).  numpy and the other oracles'
mesh makers only; nothing here asks meshcheck_oracle for an answer.

Planted pairs use small integer coordinates: every expression of the pair rule is exact on them, so geometry alone
fixes whether the two faces count as intersecting.
"""
import numpy as np

A0 = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]                     # the first face of most pairs: x, y >= 0, x + y <= 4, z = 0


def _free(t1, t2):
    return np.array(t1 + t2, np.float32), np.array([[0, 1, 2], [3, 4, 5]], np.int32)


def _mesh(verts, faces):
    return np.array(verts, np.float32), np.array(faces, np.int32)


def pairs():
    """(name, verts, faces, hit, duplicate_faces) of every planted two-face mesh."""
    out = []
    add = lambda name, m, hit, dup=0: out.append((name, m[0], m[1], hit, dup))
    # no index in common
    add('k0 transversal crossing', _free(A0, [(1, 1, -1), (1, 1, 1), (2, 2, 1)]), True)
    add('k0 boxes overlap, apart', _free(A0, [(3, 3, -1), (4, 3, 1), (3, 4, 1)]), False)
    add('k0 vertex in face interior', _free(A0, [(1, 1, 0), (1, 1, 2), (2, 1, 2)]), True)
    add('k0 edge touches edge in one point', _free(A0, [(2, -1, -1), (2, 1, 1), (2, -3, 1)]), True)
    add('k0 coplanar overlapping', _free(A0, [(1, 1, 0), (5, 1, 0), (1, 5, 0)]), True)
    add('k0 coplanar, one inside the other', _free(A0, [(1, 1, 0), (2, 1, 0), (1, 2, 0)]), True)
    add('k0 coplanar apart', _free(A0, [(3, 3, 0), (5, 3, 0), (3, 5, 0)]), False)
    add('k0 collinear edges overlapping', _free(A0, [(-1, 0, 0), (5, 0, 0), (2, 0, 3)]), True)
    add('k0 collinear edges touching at an end', _free(A0, [(4, 0, 0), (8, 0, 0), (6, 0, 3)]), True)
    add('k0 collinear edges apart', _free(A0, [(6, -2, 0), (5, -1, 0), (3, 3, 1)]), False)
    # one index in common (vertex 0)
    add('k1 fan neighbours', _mesh(A0 + [(-4, 0, 1), (0, -4, 1)], [[0, 1, 2], [0, 3, 4]]), False)
    add('k1 opposite edge piercing', _mesh(A0 + [(1, 1, -2), (1, 1, 2)], [[0, 1, 2], [0, 3, 4]]), True)
    add('k1 coplanar overlapping sectors', _mesh(A0 + [(4, 2, 0), (2, 4, 0)], [[0, 1, 2], [3, 0, 4]]), True)
    # two indices in common (the edge 0 - 1)
    add('k2 right dihedral angle', _mesh(A0 + [(0, 0, 4)], [[0, 1, 2], [1, 0, 3]]), False)
    add('k2 flat, apexes on opposite sides', _mesh(A0 + [(0, -4, 0)], [[0, 1, 2], [1, 0, 3]]), False)
    add('k2 folded flat onto its neighbour', _mesh(A0 + [(1, 2, 0)], [[0, 1, 2], [0, 1, 3]]), True)
    add('k2 folded flat, stored the other way', _mesh(A0 + [(1, 2, 0)], [[2, 0, 1], [3, 1, 0]]), True)
    # three
    add('k3 duplicate face', _mesh(A0, [[0, 1, 2], [2, 1, 0]]), False, 1)
    # a face without area takes no part
    add('zero-area face through another', _free(A0, [(1, 1, -1), (1, 1, 1), (1, 1, 3)]), False)
    return out


CUBE_FACES = [[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 7, 3], [2, 6, 7], [0, 6, 2],
              [0, 4, 6], [1, 3, 7], [1, 7, 5]]


def cube(side=2.0, origin=(0.0, 0.0, 0.0)):
    """8 vertices (index = x + 2 y + 4 z of the corner bits), 12 faces seen counter-clockwise from outside."""
    v = np.array([[(i >> 0) & 1, (i >> 1) & 1, (i >> 2) & 1] for i in range(8)], np.float32) * np.float32(side)
    return v + np.asarray(origin, np.float32), np.array(CUBE_FACES, np.int32)


def unwelded(m):
    """Every face with three vertices of its own."""
    v, f = m
    return np.ascontiguousarray(v[f.reshape(-1)]), np.arange(3 * len(f), dtype=np.int32).reshape(-1, 3)


def merge(*meshes):
    vs, fs, n = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + n)
        n += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def two_cubes_sharing_an_edge():
    """Unwelded: the cubes [0, 2]^3 and [2, 4]^2 x [0, 2] meet in the edge x = y = 2."""
    return merge(cube(2.0), cube(2.0, (2.0, 2.0, 0.0)))


def cube_one_face_flipped():
    v, f = cube(2.0)
    f = f.copy()
    f[5] = f[5][::-1]
    return v, f


def cube_one_face_removed():
    v, f = cube(2.0)
    return v, np.delete(f, 7, axis=0)


def strip(n):
    """n faces of a zig-zag strip over n + 2 vertices in general position (a gentle twist)."""
    i = np.arange(n + 2)
    v = np.stack([0.5 * i, (i % 2) * 1.0 + 0.013 * i, 0.002 * i * i], 1).astype(np.float32)
    f = np.stack([i[:-2], i[1:-1], i[2:]], 1)
    f[1::2] = f[1::2][:, [1, 0, 2]]
    return v, f.astype(np.int32)


def general():
    """(name, (verts, faces)) of the general-position shapes; made once per process."""
    if not _general:
        import mc_oracle as M
        import simplify_oracle as S
        import winding_oracle as W
        for name, m in W.shapes()[:4]:
            _general.append((name, (np.asarray(m[0], np.float32), np.asarray(m[1], np.int32))))
        _general.append(('random_signs', M.marching_cubes(M.random_signs(12))))
        v, f, _ = S.simplify(*M.marching_cubes(M.torus(32)), cells=10)
        _general.append(('simplified_torus', (v, f)))
    return list(_general)


_general = []
