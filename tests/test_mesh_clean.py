"""CPU-side pins of the component oracle (tests/cc_oracle.py) and of the no-GPU behaviour of the clean path
(octfusion_amd.mesh.components / largest_component; export_mesh clean=True, octfusion_model_union.py:459-467)."""
import numpy as np
import pytest
import torch

import cc_oracle as C
import mc_oracle as M


def _mesh(field):
    return M.marching_cubes(field)


FIELDS = {'sphere': lambda: M.sphere(32), 'torus': lambda: M.torus(40), 'gaussians48': lambda: M.gaussians(48),
          'two_spheres64': lambda: C.two_spheres(64), 'signs20': lambda: M.random_signs(20),
          'signs20_open': lambda: M.random_signs(20, border=False), 'signs32': lambda: M.random_signs(32)}


@pytest.mark.parametrize('name', sorted(FIELDS))
def test_shared_vertex_components_equal_face_adjacency(name):
    """Components by shared vertex (the kernels' contract) equal components by face adjacency across shared edges on
    every mesher output here: the mesher makes no bow-tie vertices."""
    v, f = _mesh(FIELDS[name]())
    cv = C.labels(len(v), f)
    assert (cv >= 0).all()                                  # the mesher leaves no vertex unused
    by_vertex = cv[f[:, 0]]
    assert (cv[f] == by_vertex[:, None]).all()
    assert C.same_partition(by_vertex, C.labels_by_edge(f))
    # numbered by lowest vertex id: first appearances ascend
    first = [int(np.argmax(cv == k)) for k in range(int(cv.max()) + 1)]
    assert first == sorted(first)


@pytest.mark.parametrize('name', sorted(FIELDS))
def test_against_trimesh_exactly_two_rule(name):
    """trimesh's face_adjacency keeps only edges that exactly two faces share.  On meshes whose edges all have two
    faces (sphere, torus, gaussians, two_spheres) that is the same partition.  The random-sign lattices have edges
    shared by four faces (34 of 29 072 at R = 20), which connect nothing for trimesh: it splits further -- 96 against
    79 components on random_signs(20), 136 against 112 without border, 427 against 323 on random_signs(32) -- and
    its partition refines ours."""
    v, f = _mesh(FIELDS[name]())
    ours = C.labels(len(v), f)[f[:, 0]]
    tm = C.labels_by_edge(f, exactly_two=True)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    shared = np.unique(e, axis=0, return_counts=True)[1]
    assert C.refines(tm, ours)
    if name.startswith('signs'):
        assert shared.max() == 4
        want = {'signs20': (79, 96), 'signs20_open': (112, 136), 'signs32': (323, 427)}[name]
        assert (int(ours.max()) + 1, int(tm.max()) + 1) == want
    else:
        assert shared.max() == 2 and C.same_partition(ours, tm)


def test_component_counts_of_the_issue_table():
    v, f = _mesh(C.two_spheres(64))
    t = C.table(v, f)
    assert (len(v), len(f), len(t['n_verts'])) == (4558, 9108, 2)
    assert np.allclose(np.sort(C.extents(t))[::-1], [0.800, 0.360], atol=2e-3)
    v, f = _mesh(C.rod_and_ball(96))
    t = C.table(v, f)
    assert (len(v), len(f), len(t['n_verts'])) == (12214, 24420, 2)
    assert np.allclose(np.sort(C.extents(t))[::-1], [1.600, 0.900], atol=2e-3)
    assert int(t['n_verts'].sum()) == len(v) and int(t['n_faces'].sum()) == len(f)


def test_winner_of_two_spheres_is_a_closed_sphere():
    v, f = _mesh(C.two_spheres(64))
    cv, cf, k = C.clean(v, f)
    assert k == 2 and len(cf) < len(f)
    assert M.directed_edge_balance(cf) and M.euler(cv, cf) == 2 and M.signed_volume(cv, cf) > 0
    assert int(cf.max()) == len(cv) - 1 and len(np.unique(cf)) == len(cv)
    assert abs(float((cv.max(0) - cv.min(0)).max()) - 0.8) < 2e-3


def test_rod_and_ball_winner_is_not_the_component_with_most_faces():
    v, f = _mesh(C.rod_and_ball(96))
    t = C.table(v, f)
    w = C.select(t)
    assert w != int(np.argmax(t['n_faces']))
    assert sorted(t['n_faces'].tolist()) == [2768, 21652] and int(t['n_faces'][w]) == 2768


def test_tie_goes_to_the_lowest_vertex_id():
    v, f = C.tetra_pair()
    t = C.table(v, f)
    e = C.extents(t)
    assert len(e) == 2 and e[0] == e[1] == np.float32(1.0)
    assert C.select(t) == 0
    cv, cf, _ = C.clean(v, f)
    assert np.array_equal(cv, v[:4]) and np.array_equal(cf, f[:4])
    # the copies swapped: still the one that holds vertex 0
    v2 = np.concatenate([v[4:], v[:4]])
    cv2, _, _ = C.clean(v2, f)
    assert np.array_equal(cv2, v2[:4])


def test_unused_vertices_and_empty_meshes():
    v, f = C.tetra_pair()
    v = np.concatenate([np.full((1, 3), 9, np.float32), v])          # vertex 0 is used by no face
    t = C.table(v, f + 1)
    assert t['comp_of_vert'][0] == -1 and len(t['n_verts']) == 2 and t['n_verts'].tolist() == [4, 4]
    assert float(t['bbox_max'].max()) == 5.0                          # the stray vertex is in no box
    e = C.table(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert len(e['n_verts']) == 0 and C.select(e) == -1
    assert C.clean(np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int32))[2] == 0


def test_strip_oracle():
    v, f = C.strip(2000, seed=3)
    assert len(C.table(v, f)['n_verts']) == 1
    v, f = C.strip(2000, seed=3, cut=700)
    t = C.table(v, f)
    assert sorted(t['n_faces'].tolist()) == [700, 1298] and sorted(t['n_verts'].tolist()) == [702, 1300]


def test_workspace_size_is_zero_outside_the_limits():
    from octfusion_amd import build, _lib
    build.build()
    L = _lib.lib()
    big = 2 ** 31
    assert L.ofx_mesh_cc_ws_bytes(big, 10, 1) == 0 and L.ofx_mesh_cc_ws_bytes(10, big, 1) == 0
    assert L.ofx_mesh_cc_ws_bytes(0, 10, 1) == 0 and L.ofx_mesh_cc_ws_bytes(10, 0, 1) == 0
    assert L.ofx_mesh_cc_ws_bytes(10, 10, 0) == 0
    small = L.ofx_mesh_cc_ws_bytes(1000, 2000, 2)
    assert 0 < small < 1 << 20
    # 12 V for the forest, its flags and their scan, then the larger of 24 min(V, F) and 8 F
    V, F = 18_000_000, 31_400_000
    n = L.ofx_mesh_cc_ws_bytes(V, F, 1)
    assert 12 * V + 24 * V <= n <= 12 * V + 24 * V + (1 << 20)
    assert L.ofx_mesh_cc_ws_bytes(big - 1, big - 1, 8) > 0


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_clean_fails_loudly_without_gpu():
    from octfusion_amd import _lib, mesh
    v, f = C.tetra_pair()
    m = [(torch.from_numpy(v), torch.from_numpy(f))]
    with pytest.raises(_lib.OfxError):
        mesh.largest_component(m)
    with pytest.raises(_lib.OfxError):
        mesh.components(m)
    with pytest.raises(_lib.OfxError):
        mesh.marching_cubes(torch.zeros(1, 8, 8, 8), clean=True)


def test_generate_clean_without_mesh_raises(tmp_path):
    from octfusion_amd import generate as G
    with pytest.raises(ValueError, match='--clean needs --mesh'):
        G.main(['--config', 'snet_uncond', '--shapes', '1', '--clean', '--out', str(tmp_path)])


def test_evaluate_help_says_what_clean_covers(capsys):
    from octfusion_amd import evaluate as E
    with pytest.raises(SystemExit):
        E.main(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert '--clean' in text and 'no effect on .npy' in text
