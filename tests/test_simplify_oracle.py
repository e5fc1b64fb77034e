"""The numpy restatement of the vertex-clustering rule (tests/simplify_oracle.py) on meshes whose answers are known:
closed surfaces stay closed and keep their Euler characteristic, every vertex stays in its cell, the face order of the
input does not matter beyond summation order.  And the product refuses to run without a GPU."""
import numpy as np
import pytest
import torch

import mc_oracle as M
import simplify_oracle as S


def tol(verts):
    """One fp32 ulp at the mesh's largest coordinate (the bound of tests/test_gpu_simplify.py)."""
    return float(np.spacing(np.float32(np.abs(verts).max())))


@pytest.fixture(scope='module')
def sphere():
    return M.marching_cubes(M.sphere(32))


@pytest.fixture(scope='module')
def torus():
    return M.marching_cubes(M.torus(32))


def inside_cells(verts, d):
    lo, h = d['lo'], d['h']
    t = tol(verts)                       # the one rounding to fp32
    box_lo, box_hi = lo + d['cell'] * h, lo + (d['cell'] + 1) * h
    assert (d['x64'] >= box_lo - 1e-12 * np.abs(box_lo)).all() and (d['x64'] <= box_hi + 1e-12 * np.abs(box_hi)).all()
    return box_lo, box_hi, t


@pytest.mark.parametrize('cells', [4, 8, 13])
def test_sphere_stays_closed(sphere, cells):
    v, f = sphere
    assert len(f) == 2976
    d = {}
    ov, of, st = S.simplify(v, f, cells=cells, detail=d)
    assert ov.dtype == np.float32 and of.dtype == np.int32
    assert 0 < len(of) < len(f) and of.min() == 0 and of.max() == len(ov) - 1
    assert M.directed_edge_balance(of) and M.euler(ov, of) == 2
    assert st['clusters'] == len(ov) + st['clusters_unused']
    assert st['faces_collapsed'] + st['faces_duplicate'] + len(of) == len(f)
    box_lo, box_hi, t = inside_cells(v, d)
    assert (ov >= box_lo - t).all() and (ov <= box_hi + t).all()
    r = np.linalg.norm(ov.astype(np.float64) - np.array([0.013, -0.021, 0.007]), axis=1)
    assert 0.95 * 0.5 < r.min() and r.max() < 1.05 * 0.5
    assert M.signed_volume(ov, of) > 0           # the winding survived


@pytest.mark.parametrize('cells', [8, 13])
def test_torus_keeps_its_hole(torus, cells):
    v, f = torus
    d = {}
    ov, of, st = S.simplify(v, f, cells=cells, detail=d)
    assert M.directed_edge_balance(of) and M.euler(ov, of) == 0
    box_lo, box_hi, t = inside_cells(v, d)
    assert (ov >= box_lo - t).all() and (ov <= box_hi + t).all()


@pytest.mark.parametrize('cells', [4, 8])
def test_reversed_face_order(sphere, cells):
    v, f = sphere
    ov, of, st = S.simplify(v, f, cells=cells)
    rv, rf, rst = S.simplify(v, f[::-1], cells=cells)
    assert rst == st and rv.shape == ov.shape and len(rf) == len(of)
    assert np.abs(rv.astype(np.float64) - ov.astype(np.float64)).max() <= tol(v)
    # no duplicates here, so the surviving faces are the same set, listed backwards
    assert np.array_equal(rf[::-1], of)


def test_cells_one_and_empty_inputs(sphere):
    v, f = sphere
    ov, of, st = S.simplify(v, f, cells=1)
    assert ov.shape == (0, 3) and of.shape == (0, 3)
    assert st == dict(clusters=1, faces_collapsed=len(f), faces_duplicate=0, clusters_unused=1)
    ov, of, st = S.simplify(v[:3], np.zeros((0, 3), np.int32), cells=4)
    assert ov.shape == (0, 3) and of.shape == (0, 3) and st['clusters'] == 0
    with pytest.raises(ValueError):
        S.simplify(v, f)
    with pytest.raises(ValueError):
        S.simplify(v, f, cells=4, cell_size=0.1)
    with pytest.raises(ValueError, match='overflow'):
        S.simplify(v, f, cell_size=1e-4)


def test_duplicates_and_unused_clusters():
    v, f = M.marching_cubes(M.random_signs(12))
    ov, of, st = S.simplify(v, f, cells=8)
    assert st['faces_duplicate'] > 0 and st['clusters_unused'] > 0
    assert len(np.unique(S.rotate(of.astype(np.int64)), axis=0)) == len(of)
    assert len(np.unique(of)) == len(ov)


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_simplify_fails_loudly_without_gpu():
    from octfusion_amd import _lib, simplify
    with pytest.raises(_lib.OfxError):
        simplify.simplify([(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))], cells=4)
