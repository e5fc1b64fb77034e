"""The meshes of the smoothing tests that tests/meshcheck_cases.py does not already make.  numpy and the other oracles'
mesh makers only; nothing here asks smooth_oracle for an answer."""
import numpy as np

import meshcheck_cases as C

TETRA = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32),
         np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32))


def fan(n, centre, rim_z=0.0):
    """n triangles around vertex 0 (the centre): its row has n entries.  The rim is a regular n-gon of radius 1 in
    z = rim_z and is the boundary."""
    a = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([[centre], np.stack([np.cos(a), np.sin(a), np.full(n, rim_z)], 1)]).astype(np.float32)
    f = np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 1 + (np.arange(n) + 1) % n], 1).astype(np.int32)
    return v, f


def noisy_icosphere(seed=0):
    """162 vertices, 320 faces; every vertex of the unit icosphere scaled by 1 + 0.05 N(0, 1), rounded to fp32."""
    import mesh2sdf_oracle as O
    v, f = O.icosphere(2)
    r = 1 + 0.05 * np.random.default_rng(seed).standard_normal(len(v))
    return (np.asarray(v, np.float64) * r[:, None]).astype(np.float32), np.asarray(f, np.int32)


def defects():
    """The cube with two index-degenerate faces, a duplicate of face 0 (reversed), a face without area on the edge
    0 - 1 (through vertex 8, its midpoint) and two vertices no face uses: 9, and 10 which holds NaN."""
    v, f = C.cube(2.0)
    v = np.concatenate([v, [[1, 0, 0], [7, 7, 7], [np.nan, np.nan, np.nan]]]).astype(np.float32)
    f = np.concatenate([[[4, 4, 5]], f[:6], [[3, 2, 0], [0, 1, 8]], f[6:], [[6, 7, 6]]]).astype(np.int32)
    return v, f


def ripple_lattice(R=32):
    """[R, R, R] fp32: a sphere of radius 0.6 with 0.02 sin ripples, on the lattice of mc_oracle.lattice_coords."""
    import mc_oracle as M
    x, y, z = M.lattice_coords(R)
    return (np.sqrt(x * x + y * y + z * z) - 0.6 + 0.02 * np.sin(9 * x) * np.sin(7 * y) * np.sin(8 * z)).astype(np.float32)


def all_meshes():
    """(name, (verts, faces)) of every mesh of the device tests."""
    out = [('tetrahedron', TETRA), ('cube', C.cube(2.0))] + C.general()
    out += [('two_cubes_sharing_an_edge', C.two_cubes_sharing_an_edge()), ('flipped', C.cube_one_face_flipped()),
            ('removed', C.cube_one_face_removed()), ('strip7', C.strip(7)), ('unwelded', C.unwelded(C.cube(2.0))),
            ('icosphere', noisy_icosphere()), ('fan200', fan(200, (0.1, -0.2, 0.6))),
            ('fan1000', fan(1000, (-0.2, 0.1, 0.4), 0.1)), ('defects', defects())]
    return [(name, (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32))) for name, (v, f) in out]
