"""CPU checks of what the mesh entry-point tests lean on (test_gpu_mesh_entry.py, test_gpu_mesh_cc_entry.py,
test_gpu_simplify_entry.py): the extended oracles themselves, and the facts about the inputs those tests feed the
device -- established here, without a GPU."""
import numpy as np
import pytest

import cc_oracle as CO
import mc_oracle as M
import mesh_entry_util as U
import simplify_oracle as S
import voxmesh_oracle as VO
from test_gpu_mesh_entry import _cube_cases, _noise, morton_keys
from test_gpu_simplify_entry import degenerate_meshes


# ------------------------------------------------------------------------------------------------ marching cubes
@pytest.mark.parametrize('R', [2, 3, 10, 11, 16, 17])
def test_smallest_lattices_all_have_a_surface(R):
    f = _noise(3, R, R)
    f[1] = M.sphere(R) if R > 3 else -f[0]
    for b in range(3):
        v, t = M.marching_cubes(f[b])
        assert len(v) > 0 and len(t) > 0
    assert (R ** 3 + 1023) // 1024 == {2: 1, 3: 1, 10: 1, 11: 2, 16: 4, 17: 5}[R]       # 1024-point chunks


def test_the_256_cube_cases_are_the_table():
    f = _cube_cases(np.arange(256), np.random.default_rng(256).uniform(0.1, 2.0, (256, 8)))
    _, ntri = M.tables()
    for c in range(256):
        assert int(M.cube_index(f[c] < 0)[0, 0, 0]) == c
        v, t = M.marching_cubes(f[c])
        assert len(t) == ntri[c] and len(v) == len(np.unique(t)) or len(t) == 0


def test_ties_signed_zero_and_denormals_are_outside_or_inside_by_less_than():
    tiny = np.float32(1e-45)
    assert M.marching_cubes(np.full((3, 3, 3), 0.25, np.float32), level=0.25)[0].shape == (0, 3)
    z = np.full((3, 3, 3), -0.0, np.float32)
    z[1, 1, 1] = 1.0
    assert M.marching_cubes(z)[0].shape == (0, 3)                    # -0.0 < 0.0 is false
    for rest, centre in ((0.0, -1.0), (-0.0, -tiny), (tiny, -tiny)):
        f = np.full((3, 3, 3), rest, np.float32)
        f[1, 1, 1] = centre
        v, t = M.marching_cubes(f)
        assert len(v) == 6 and len(t) == 8
    assert float(tiny) > 0 and np.float32(-tiny) < np.float32(0.0)


def test_a_difference_that_overflows_puts_the_vertex_on_the_owner():
    f = np.full((2, 2, 2), 3e38, np.float32)
    f[0, 0, 0] = -3e38
    with np.errstate(over='ignore'):
        assert np.isinf(np.float32(3e38) - np.float32(-3e38))
    for g in (f, -f):
        v, t = M.marching_cubes(g, bbmin=-0.9, bbmax=0.9, scale=2.0)
        assert len(t) == 1 and np.array_equal(v, np.full((3, 3), np.float32(-0.9) * np.float32(2.0)))


def test_non_finite_cells_of_a_corner_an_edge_a_face_and_the_inside():
    for bad in (np.nan, np.inf, -np.inf):
        for p, n in (((0, 0, 0), 1), ((1, 0, 0), 2), ((1, 1, 0), 4), ((1, 1, 1), 8)):
            f = _noise(1, 4, 3)[0]
            f[p] = bad
            assert M.nonfinite_cells(f) == n


def test_batch_bounds_of_the_wrappers():
    from octfusion_amd import mesh, voxmesh
    assert mesh._max_batch(2) == mesh._max_batch(16) == 65535 and mesh._max_batch(256) == 25
    assert mesh._max_batch(512) == 3 and mesh._max_batch(32) == (2 ** 31 - 1) // (5 * 32 ** 3) < 65535
    assert voxmesh._max_batch(2) == voxmesh._max_batch(8) == 65535 and voxmesh._max_batch(256) == 5


# ------------------------------------------------------------------------------------------------ voxel meshes
def test_morton_keys_and_the_dense_special_values():
    k = morton_keys([1, 0, 0, 5], [0, 1, 0, 2], [0, 0, 1, 7], [0, 0, 3, 1], 3)
    assert k[:3].tolist() == [4, 2, 1 | (3 << 48)]                  # x, y, z in bits 2, 1, 0; the shape from bit 48
    x, y, z = 5, 2, 7
    want = sum((((x >> i) & 1) << 2 | ((y >> i) & 1) << 1 | ((z >> i) & 1)) << (3 * i) for i in range(3))
    assert int(k[3]) == want | (1 << 48)
    thr = np.float32(0.4)
    g = np.array([thr, np.nextafter(thr, np.float32(1)), np.nan, np.inf, -np.inf, 1.0], np.float32)
    assert VO.occupancy(g, thr).tolist() == [False, True, False, False, False, True]
    one = np.zeros((2, 2, 2), np.float32)
    one[1, 0, 1] = 1
    assert len(VO.unwelded(one, 0.5)[1]) == 12 and len(VO.welded(one, 0.5)[0]) == 8


# ------------------------------------------------------------------------------------------------ components
def test_tiny_batch_and_its_component_counts():
    kinds, meshes = U.tiny_batch()
    assert len(meshes) == 300 and all(kinds.count(k) >= 30 for k in U.KINDS)
    per = dict(tetra=1, pair=2, no_verts=0, no_faces=0, unused=1)
    for k, (v, f) in zip(kinds, meshes):
        tab = CO.table(v, f)
        assert len(tab['n_verts']) == per[k]
        if k == 'unused':
            assert tab['comp_of_vert'].tolist() == [-1, -1, 0, 0, 0, 0, -1]
    v, f, voff, toff = U.cat(meshes)
    assert voff[-1] == len(v) and toff[-1] == len(f) and (np.diff(voff) == 0).any() and (np.diff(toff) == 0).any()
    assert np.diff(voff).max() <= 8                                  # a wave of 64 spans eight shapes or more


def test_topologies_have_the_expected_components():
    for (v, f), k in ((U.fan(20000), 1), (U.comb(40, 60), 1), (U.reversed_strip(5000), 1),
                      (CO.strip(3000, seed=4, cut=1500), 2)):
        cv = CO.labels(len(v), f)
        assert cv.max() + 1 == k and (cv >= 0).all() and f.max() == len(v) - 1
    assert len(U.fan(20000)[1]) == 20000 and (U.fan(20000)[1][:, 0] == 0).all()
    sv, sf = U.uv_sphere()
    assert len(sv) == 2000 and len(sf) == 3900 and CO.labels(2000, sf).max() == 0 and CO.labels(2000, sf).min() == 0


def test_box_order_of_signed_zeros_denormals_and_infinities():
    tiny = np.float32(1e-45)
    vals = np.array([-np.inf, -1.0, -tiny, -0.0, 0.0, tiny, 1.0, np.inf], np.float32)
    keys = CO.order_key(vals)
    assert (np.diff(keys.astype(np.int64)) > 0).all()                # strictly ascending, -0.0 below +0.0
    assert np.array_equal(CO.order_value(keys).view(np.int32), vals.view(np.int32))
    v = np.array([[0.0, tiny, np.inf], [-0.0, -tiny, -np.inf], [0.0, 0.0, 1.0]], np.float32)
    for order in ([0, 1, 2], [1, 0, 2], [2, 1, 0]):
        tab = CO.table(v[order], np.array([[0, 1, 2]]))
        assert tab['bbox_min'].view(np.int32).tolist() == [np.array([-0.0, -tiny, -np.inf], np.float32).view(np.int32).tolist()]
        assert tab['bbox_max'].view(np.int32).tolist() == [np.array([0.0, tiny, np.inf], np.float32).view(np.int32).tolist()]


def test_extents_that_tie_in_fp32_only():
    lo, hi = np.float32(0.1), np.float32(1.1)
    assert np.float32(hi - lo) == np.float32(1.0) and float(hi) - float(lo) > 1.0
    a = U.TETRA_V * np.array([1, 0.5, 0.5], np.float32)
    b = np.array([[lo, 3, 3], [hi, 3, 3], [lo, 3.5, 3], [lo, 3, 3.5]], np.float32)
    f2 = np.concatenate([U.TETRA_F, U.TETRA_F + 4])
    assert CO.select(CO.table(np.concatenate([a, b]), f2)) == 0 == CO.select(CO.table(np.concatenate([b, a]), f2))


# ------------------------------------------------------------------------------------------------ simplification
def test_non_finite_vertices_are_refused_by_the_oracle_in_both_modes():
    v, f = U.tiny_shape('unused', np.random.default_rng(5))
    assert not S.nonfinite(v)
    for bad in (np.nan, np.inf, -np.inf):
        for at in (3, 6):                                            # a vertex a face uses, one that none uses
            w = v.copy()
            w[at, 1] = bad
            assert S.nonfinite(w)
            for kw in (dict(cells=8), dict(cell_size=0.125)):
                with pytest.raises(ValueError, match='non-finite'):
                    S.simplify(w, f, **kw)


def test_cell_sizes_that_need_1024_and_1023_cells_are_decided_without_a_tie():
    over, fits = U.OVERFLOW_CELL_SIZES
    v = U.TETRA_V
    assert np.floor((1.0 - 0.0) / over) == 1024 and np.floor(1.0 / fits) == 1023
    assert abs(1.0 / over - 1024.5) < 1e-9 and abs(1.0 / fits - 1023.5) < 1e-9          # half a cell from the next integer
    with pytest.raises(ValueError, match='grid overflow'):
        S.grid(v, cell_size=over)
    assert S.grid(v, cell_size=fits)[2].max() == 1023


def test_degenerate_boxes_go_through_the_oracle():
    meshes = degenerate_meshes()
    for kw in (dict(cells=3), dict(cells=1024), dict(cell_size=0.25)):
        _, _, st = S.simplify(*meshes[0], **kw)
        assert st == dict(clusters=1, faces_collapsed=3, faces_duplicate=0, clusters_unused=1)
        for m in meshes[1:]:
            wv, wf, _ = S.simplify(*m, **kw)
            assert np.isfinite(wv).all()
    thin = meshes[2][0]
    assert np.ptp(thin[:, 0]) == np.spacing(np.float32(1.0)) and not np.ptp(thin[:, 1:], axis=0).any()
    assert S.grid(thin, cells=1024)[2].max() == 1023


def test_gapped_offsets_cover_disjoint_ranges():
    rng = np.random.default_rng(0)
    counts = np.array([3, 0, 5, 0, 0, 2])
    off, total = U.gapped(counts, rng)
    assert off[0] == 3 and (off[1:] >= off[:-1] + counts[:-1]).all() and total >= off[-1] + counts[-1]
    assert U.rows_of(off, counts).sum() == counts.sum()
