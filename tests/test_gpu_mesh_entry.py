"""Marching cubes (csrc/ofx_mesh.hip) and the voxel meshes (csrc/ofx_voxmesh.hip) one entry point at a time through the
C ABI, against tests/mc_oracle.py and tests/voxmesh_oracle.py.  Every output is prefilled with a sentinel and sits,
like the workspace (sized exactly by the ws_bytes entry), between sentinel bands; the offsets of the emit calls leave
gaps, which must keep the sentinel; a second pass over the same workspace must give the same bytes.

    entry point             cases                                                            refusals
    ofx_mc_ws_bytes         limits of size and batch, the batch bound 65535 and the          0 outside
                            device's second grid dimension
    ofx_mc_count / _emit    lattices of 8 .. 4913 points in batches of 3, the 256 cube       OFX_EINVAL: NULLs, NaN /
                            cases, ties at the level, -0.0, denormals, levels +-0.25,         infinite level, batch 70 000
                            a difference that overflows fp32, gapped offsets around an
                            empty shape, non-finite cells, 65 535 lattices of size 2
    ofx_mc_table_host       entry by entry against the oracle's table                        NULLs
    ofx_voxmesh_ws_bytes    depth 0 / 9, the batch limits per depth                          0 outside
    ofx_voxmesh_mask_keys   a batch0 window, foreign / duplicate / too deep keys, n == 0,    NULLs, n < 0, batch0 < 0
                            a refill with fewer keys
    ofx_voxmesh_mask_dense  ties at the threshold, NaN, +-inf, the grid boundary,            NULLs, NaN threshold,
                            65 535 grids of depth 1                                          batch 65 536
    ofx_voxmesh_count/_emit depths 1, 2, 3, 4 and 8, welded and not, a single cell,          NULLs
                            gapped offsets around an empty shape

Indices, counts, masks and voxel coordinates are compared exactly, marching-cubes vertices within
1e-6 (bbmax - bbmin) |scale| as in test_gpu_mesh.py.
"""
import numpy as np
import pytest
import torch

import mc_oracle as M
import voxmesh_oracle as VO
from mesh_entry_util import (INT32_MAX, Guarded, _call, _refused, gapped, lib, max_grid_dim_y, rows_of, settled, up,
                             workspace)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

F32, I32, I64 = torch.float32, torch.int32, torch.int64
MAX_BATCH = 65535


# =============================================================================================== marching cubes
class McRun:
    """count, readback, emit of a batch [B, R, R, R] through the raw entry points."""

    def __init__(self, fields, level=0.0, bbmin=-0.9, bbmax=0.9, scale=1.0, gaps=None):
        fields = np.ascontiguousarray(fields, np.float32)
        self.fields, self.B, self.R = fields, fields.shape[0], fields.shape[1]
        self.level, self.bbmin, self.bbmax, self.scale = level, bbmin, bbmax, scale
        self.step = (float(bbmax) - float(bbmin)) / self.R
        nbytes = lib().ofx_mc_ws_bytes(self.B, self.R)
        assert nbytes > 0
        self.ws = workspace(nbytes)
        self.sdf = up(fields, F32)
        self.counts = Guarded(self.B, I64, cols=3)
        self.count()
        c = self.c = self.counts.get()
        rng = np.random.default_rng(gaps) if gaps is not None else None
        if rng is None:
            self.voff, nvr = np.cumsum(c[:, 0]) - c[:, 0], int(c[:, 0].sum())
            self.toff, ntr = np.cumsum(c[:, 1]) - c[:, 1], int(c[:, 1].sum())
        else:
            self.voff, nvr = gapped(c[:, 0], rng)
            self.toff, ntr = gapped(c[:, 1], rng)
        self.verts, self.faces = Guarded(max(nvr, 1), F32, cols=3), Guarded(max(ntr, 1), I32, cols=3)
        self.offs = up(np.stack([self.voff, self.toff]), I64)
        self.emit()

    def count(self):
        _call('ofx_mc_count', self.sdf.data_ptr(), self.B, self.R, self.level, self.ws.ptr, self.counts.ptr)

    def emit(self):
        _call('ofx_mc_emit', self.sdf.data_ptr(), self.B, self.R, self.level, self.step, self.bbmin, self.scale,
              self.ws.ptr, self.offs.data_ptr(), self.offs.data_ptr() + 8 * self.B, self.verts.ptr, self.faces.ptr)

    def shape(self, b):
        v, f = self.verts.get(), self.faces.get()
        return (v[self.voff[b]:self.voff[b] + self.c[b, 0]], f[self.toff[b]:self.toff[b] + self.c[b, 1]])

    def check(self, shapes=None):
        """Every (or the given) shape against the oracle; guards, gaps; a second pass gives the same bytes."""
        tol = 1e-6 * (self.bbmax - self.bbmin) * abs(self.scale)
        assert self.ws.bands_intact() and self.counts.bands_intact()
        for b in (range(self.B) if shapes is None else shapes):
            wv, wf = M.marching_cubes(self.fields[b], self.level, self.bbmin, self.bbmax, self.scale)
            assert self.c[b, 0] == len(wv) and self.c[b, 1] == len(wf), b
            assert self.c[b, 2] == M.nonfinite_cells(self.fields[b]), b
            gv, gf = self.shape(b)
            assert np.array_equal(gf, wf), b
            if len(wv):
                assert np.isfinite(gv).all() and np.abs(gv.astype(np.float64) - wv).max() <= tol, b
        vm, tm = rows_of(self.voff, self.c[:, 0]), rows_of(self.toff, self.c[:, 1])
        vrows, trows = np.ones(self.verts.n // 3, bool), np.ones(self.faces.n // 3, bool)
        vrows[:len(vm)] = ~vm
        trows[:len(tm)] = ~tm
        assert self.verts.is_sentinel(vrows) and self.faces.is_sentinel(trows)      # the gaps, and the tail
        first = (self.counts.raw(), self.verts.raw(), self.faces.raw())
        for g in (self.counts, self.verts, self.faces):
            g.reset()
        self.count()
        self.emit()
        again = (self.counts.raw(), self.verts.raw(), self.faces.raw())
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
        assert self.ws.bands_intact()
        return self


def _noise(B, R, seed):
    return np.random.default_rng(seed).standard_normal((B, R, R, R)).astype(np.float32)


@pytest.mark.parametrize('R', [2, 3, 10, 11, 16, 17])
def test_mc_smallest_lattices(R):
    """R^3 = 8, 27, 1000, 1331, 4096, 4913: below one 1024-point chunk, just under and over one, exactly four and just
    over four (a chunk then ends in the middle of a row and the last block is nearly idle)."""
    f = _noise(3, R, R)
    f[1] = M.sphere(R) if R > 3 else -f[0]
    run = McRun(f, gaps=R).check()
    assert run.c[:, 0].min() > 0 and run.c[:, 1].min() > 0


def _cube_cases(signs_inside, mag):
    """[n, 2, 2, 2] lattices: corner c = dx*4 + dy*2 + dz is inside (negative) iff bit c of its case is set."""
    c = np.arange(8)
    inside = ((np.asarray(signs_inside)[:, None] >> c[None, :]) & 1).astype(bool)
    return np.where(inside, -mag, mag).astype(np.float32).reshape(-1, 2, 2, 2)


def test_mc_all_256_cube_cases_and_the_table():
    rng = np.random.default_rng(256)
    f = _cube_cases(np.arange(256), rng.uniform(0.1, 2.0, (256, 8)))
    run = McRun(f, gaps=7).check()
    tri, ntri = M.tables()
    assert np.array_equal(run.c[:, 1], ntri.astype(np.int64))
    # the host table, entry by entry
    import ctypes
    t = (ctypes.c_int8 * (256 * 16))()
    n = (ctypes.c_uint8 * 256)()
    assert lib().ofx_mc_table_host(ctypes.addressof(t), ctypes.addressof(n)) == 0
    assert np.array_equal(np.frombuffer(t, np.int8).reshape(256, 16), tri)
    assert np.array_equal(np.frombuffer(n, np.uint8), ntri)
    assert lib().ofx_mc_table_host(None, ctypes.addressof(n)) != 0 and lib().ofx_mc_table_host(ctypes.addressof(t), None) != 0


def test_mc_ties_zeros_denormals_and_levels():
    tiny = np.float32(1e-45)                                       # the smallest denormal
    assert tiny > 0 and tiny == np.nextafter(np.float32(0), np.float32(1))
    # corners exactly at the level are outside: a lattice of nothing but the level has no surface
    flat = np.full((1, 3, 3, 3), 0.25, np.float32)
    assert McRun(flat, level=0.25).check().c.sum() == 0
    # -0.0 at level 0.0 is outside (not < 0); next to +1 there is no crossing either
    z = np.full((1, 3, 3, 3), -0.0, np.float32)
    z[0, 1, 1, 1] = 1.0
    assert McRun(z).check().c.sum() == 0
    # one inside corner among corners at the level, at -0.0 and at denormals of both signs
    f = np.zeros((4, 3, 3, 3), np.float32)
    f[0] = 0.0
    f[0, 1, 1, 1] = -1.0                                           # neighbours tie with the level: t = 1
    f[1] = -0.0
    f[1, 1, 1, 1] = -tiny                                          # a denormal is inside
    f[2] = tiny                                                    # ... and outside
    f[2, 1, 1, 1] = -tiny
    f[3] = _noise(1, 3, 11)[0]
    f[3, 0, 1, 2] = 0.0
    run = McRun(f, gaps=3).check()
    assert run.c[:3, 0].tolist() == [6, 6, 6] and run.c[:3, 1].tolist() == [8, 8, 8]
    # a negative level, with ties at it
    g = _noise(2, 4, 5)
    g[0, 1, 2, 1] = g[1, 0, 0, 0] = -0.5
    McRun(g, level=-0.5, gaps=1).check()
    # one field at +-0.25 against the oracle: the face count moves with the level
    s = np.stack([M.gaussians(16), M.torus(16)])
    lo, hi = McRun(s, level=-0.25, gaps=2).check(), McRun(s, level=0.25, gaps=2).check()
    assert (lo.c[:, 1] != hi.c[:, 1]).all()


def test_mc_difference_that_overflows_fp32():
    """v0 = -3e38, v1 = 3e38: v1 - v0 is +inf in fp32, t = (level - v0) / inf = 0 and the vertex is the owner point."""
    f = np.full((2, 2, 2, 2), 3e38, np.float32)
    f[0, 0, 0, 0] = -3e38                                          # the owner of three crossing edges
    f[1] = -f[0]                                                   # v1 - v0 = -inf: t = -0
    run = McRun(f, bbmin=-0.9, bbmax=0.9, scale=2.0).check()
    assert run.c[:, 0].tolist() == [3, 3] and run.c[:, 1].tolist() == [1, 1]
    for b in range(2):
        v, _ = run.shape(b)
        assert np.array_equal(v, np.full((3, 3), np.float32(np.float32(-0.9) * np.float32(2.0))))


def test_mc_gapped_offsets_around_an_empty_shape():
    R = 11
    f = np.stack([M.sphere(R), np.full((R, R, R), 1.0, np.float32), M.torus(R), np.full((R, R, R), -1.0, np.float32)])
    run = McRun(f, gaps=11).check()
    assert run.c[1].tolist() == [0, 0, 0] and run.c[3].tolist() == [0, 0, 0] and run.c[2, 1] > 0
    assert run.voff[0] > 0 and run.toff[0] > 0                     # the first shape does not start at 0 either


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_mc_non_finite_cells(bad):
    """A non-finite value at a lattice corner, on an edge, in a face and inside touches 1, 2, 4 and 8 cells."""
    R = 4
    f = _noise(4, R, 3)
    for b, p in enumerate([(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)]):
        f[b][p] = bad
    run = McRun(f, gaps=4)
    assert run.c[:, 2].tolist() == [1, 2, 4, 8] == [M.nonfinite_cells(x) for x in f]
    assert run.ws.bands_intact() and run.verts.bands_intact() and run.faces.bands_intact()


def test_mc_ws_bytes_limits_and_the_grid_dimension():
    ws = lib().ofx_mc_ws_bytes
    assert ws(1, 1) == 0 and ws(1, 513) == 0 and ws(0, 8) == 0 and ws(-1, 8) == 0
    assert ws(1, 2) > 0 and ws(1, 512) > 0
    for size in (32, 64, 512):                                     # the int32 scan bounds the batch of large lattices
        top = INT32_MAX // (5 * size ** 3)
        assert 1 <= top < MAX_BATCH and ws(top, size) > 0 and ws(top + 1, size) == 0
    for size in (2, 3, 16):                                        # the grid bounds the batch of small ones
        assert INT32_MAX // (5 * size ** 3) > MAX_BATCH
        assert ws(MAX_BATCH, size) > 0 and ws(MAX_BATCH + 1, size) == 0
    assert ws(70000, 2) == 0
    assert MAX_BATCH <= max_grid_dim_y()                           # what one launch can take, from the device


def test_mc_refusals():
    R, B = 5, 2
    sdf = up(_noise(B, R, 0), F32)
    ws = workspace(lib().ofx_mc_ws_bytes(B, R))
    counts, verts, faces = Guarded(B, I64, cols=3), Guarded(64, F32, cols=3), Guarded(64, I32, cols=3)
    offs = up(np.zeros(2 * B), I64)
    good_c = [sdf.data_ptr(), B, R, 0.0, ws.ptr, counts.ptr]
    good_e = [sdf.data_ptr(), B, R, 0.0, 0.36, -0.9, 1.0, ws.ptr, offs.data_ptr(), offs.data_ptr(), verts.ptr,
              faces.ptr]

    def variants(good, at):
        for i, v in at:
            a = list(good)
            a[i] = v
            yield a
    for a in variants(good_c, [(0, None), (4, None), (5, None), (3, float('nan')), (3, float('inf')),
                               (3, float('-inf')), (1, 0), (1, 70000), (2, 1), (2, 513)]):
        _refused('ofx_mc_count', *a)
    for a in variants(good_e, [(0, None), (7, None), (8, None), (9, None), (10, None), (11, None), (3, float('nan')),
                               (3, float('inf')), (1, 0), (1, 70000), (2, 1), (2, 513)]):
        _refused('ofx_mc_emit', *a)
    settled(ws, counts, verts, faces)


def test_mc_largest_batch():
    """70 000 lattices of size 2 are one more than a launch can take: refused.  The largest accepted batch, 65 535,
    is meshed like the oracle: the counts of every shape, the meshes of a few hundred."""
    rng = np.random.default_rng(70000)
    cases = rng.integers(0, 256, 70000)
    f = _cube_cases(cases, rng.uniform(0.1, 2.0, (70000, 8)))
    assert f.nbytes == 70000 * 32
    sdf = up(f, F32)
    small_ws, counts = workspace(lib().ofx_mc_ws_bytes(MAX_BATCH, 2)), Guarded(70000, I64, cols=3)
    assert lib().ofx_mc_ws_bytes(70000, 2) == 0
    _refused('ofx_mc_count', sdf.data_ptr(), 70000, 2, 0.0, small_ws.ptr, counts.ptr)
    settled(small_ws, counts)
    run = McRun(f[:MAX_BATCH], gaps=5)
    _, ntri = M.tables()
    inside = f[:MAX_BATCH] < 0
    cross = ((inside[:, 1:] != inside[:, :-1]).sum((1, 2, 3)) + (inside[:, :, 1:] != inside[:, :, :-1]).sum((1, 2, 3)) +
             (inside[:, :, :, 1:] != inside[:, :, :, :-1]).sum((1, 2, 3)))
    assert np.array_equal(run.c[:, 0], cross) and np.array_equal(run.c[:, 1], ntri[cases[:MAX_BATCH]].astype(np.int64))
    assert not run.c[:, 2].any()
    sample = np.concatenate([[0, 1, MAX_BATCH - 2, MAX_BATCH - 1], rng.integers(0, MAX_BATCH, 296)])
    run.check(shapes=sample.tolist())


# =============================================================================================== voxel meshes
def morton_keys(x, y, z, b, depth):
    x, y, z, b = (np.asarray(a, np.int64) for a in (x, y, z, b))
    k = np.zeros_like(x)
    for i in range(depth):
        k |= (((x >> i) & 1) << (3 * i + 2)) | (((y >> i) & 1) << (3 * i + 1)) | (((z >> i) & 1) << (3 * i))
    return k | (b << 48)


class VmRun:
    """fill (given), count, readback, emit of B grids of 2^depth through the raw entry points."""

    def __init__(self, B, depth, weld, fill, gaps=None):
        self.B, self.depth, self.weld, self.R = B, depth, int(weld), 1 << depth
        nbytes = lib().ofx_voxmesh_ws_bytes(B, depth, self.weld)
        assert nbytes > 0
        self.ws = workspace(nbytes)
        self.fill = fill
        fill(self.ws)
        self.counts = Guarded(B, I64, cols=2)
        self.count()
        c = self.c = self.counts.get()
        self.nv = c[:, 1] if self.weld else 4 * c[:, 0]
        self.nt = 2 * c[:, 0]
        rng = np.random.default_rng(gaps) if gaps is not None else None
        if rng is None:
            self.voff, nvr = np.cumsum(self.nv) - self.nv, int(self.nv.sum())
            self.toff, ntr = np.cumsum(self.nt) - self.nt, int(self.nt.sum())
        else:
            self.voff, nvr = gapped(self.nv, rng)
            self.toff, ntr = gapped(self.nt, rng)
        self.verts, self.faces = Guarded(max(nvr, 1), F32, cols=3), Guarded(max(ntr, 1), I32, cols=3)
        self.offs = up(np.stack([self.voff, self.toff]), I64)
        self.emit()

    def count(self):
        _call('ofx_voxmesh_count', self.B, self.depth, self.weld, self.ws.ptr, self.counts.ptr)

    def emit(self):
        _call('ofx_voxmesh_emit', self.B, self.depth, self.weld, self.ws.ptr, self.offs.data_ptr(),
              self.offs.data_ptr() + 8 * self.B, self.verts.ptr, self.faces.ptr)

    def check(self, occ, shapes=None, want=None):
        """occ: boolean [B, R, R, R], the occupancy the fill must have produced."""
        assert self.ws.bands_intact() and self.counts.bands_intact()
        v, f = self.verts.get(), self.faces.get()
        for b in (range(self.B) if shapes is None else shapes):
            wv, wf = want[b] if want is not None else VO.mesh(occ[b].astype(np.float32), 0.5, weld=bool(self.weld))
            assert self.c[b, 0] * 2 == len(wf) and self.nv[b] == len(wv), b
            if not self.weld:
                assert self.c[b, 1] == 0
            assert np.array_equal(v[self.voff[b]:self.voff[b] + self.nv[b]], wv), b       # exact coordinates
            assert np.array_equal(f[self.toff[b]:self.toff[b] + self.nt[b]], wf), b
        vm, tm = rows_of(self.voff, self.nv), rows_of(self.toff, self.nt)
        vrows, trows = np.ones(self.verts.n // 3, bool), np.ones(self.faces.n // 3, bool)
        vrows[:len(vm)] = ~vm
        trows[:len(tm)] = ~tm
        assert self.verts.is_sentinel(vrows) and self.faces.is_sentinel(trows)
        first = (self.counts.raw(), self.verts.raw(), self.faces.raw())
        for g in (self.counts, self.verts, self.faces):
            g.reset()
        self.fill(self.ws)
        self.count()
        self.emit()
        assert all(np.array_equal(a, b) for a, b in zip(first, (self.counts.raw(), self.verts.raw(), self.faces.raw())))
        assert self.ws.bands_intact()
        return self


def dense_fill(grids, threshold):
    grids = np.ascontiguousarray(grids, np.float32)
    B, depth = grids.shape[0], int(grids.shape[1]).bit_length() - 1
    t = up(grids, F32)
    return lambda ws: _call('ofx_voxmesh_mask_dense', t.data_ptr(), B, depth, threshold, ws.ptr)


def keys_fill(keys, batch0, B, depth):
    t = up(keys, I64)
    n = len(keys)
    return lambda ws: _call('ofx_voxmesh_mask_keys', t.data_ptr(), n, batch0, B, depth, ws.ptr)


@pytest.mark.parametrize('weld', [0, 1])
@pytest.mark.parametrize('depth', [1, 2, 3, 4])
def test_voxmesh_random_grids_single_cell_and_an_empty_shape(depth, weld):
    R = 1 << depth
    g = np.stack([VO.random_grid(R, 0.5, depth), np.zeros((R, R, R), np.float32), VO.random_grid(R, 0.2, 10 + depth),
                  np.zeros((R, R, R), np.float32), np.ones((R, R, R), np.float32)])
    g[3, R - 1, 0, R - 1] = 1                                      # a single cell, in a corner of the grid
    run = VmRun(5, depth, weld, dense_fill(g, 0.5), gaps=depth).check(g > 0.5)
    assert run.c[1].tolist() == [0, 0] and run.c[3, 0] == 6 and run.c[4, 0] == 6 * R * R
    assert run.c[3, 1] == (8 if weld else 0)


@pytest.fixture(scope='module')
def deep():
    """Depth 8 through the keys: 3000 random cells and the eight corners of the grid, in shape 1 of a window of 2."""
    rng = np.random.default_rng(8)
    R = 256
    xyz = np.concatenate([rng.integers(0, R, (3000, 3)), np.array([[i, j, k] for i in (0, R - 1) for j in (0, R - 1)
                                                                    for k in (0, R - 1)])])
    occ = np.zeros((R, R, R), bool)
    occ[xyz[:, 0], xyz[:, 1], xyz[:, 2]] = True
    g = occ.astype(np.float32)
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v, f = VO.unwelded(g, 0.5)
    return xyz, {0: [empty, (v, f)], 1: [empty, VO.weld(v, f, R)]}


@pytest.mark.parametrize('weld', [0, 1])
def test_voxmesh_depth_8(deep, weld):
    xyz, want = deep
    keys = morton_keys(xyz[:, 0], xyz[:, 1], xyz[:, 2], np.full(len(xyz), 6), 8)
    run = VmRun(2, 8, weld, keys_fill(keys, 5, 2, 8), gaps=8).check(None, want=want[weld])
    assert run.c[0].tolist() == [0, 0] and run.c[1, 0] > 6 * 2000


def test_voxmesh_mask_keys_window_duplicates_and_refill():
    depth, R, B, b0 = 3, 8, 3, 4
    rng = np.random.default_rng(3)
    n = 400
    x, y, z = rng.integers(0, R, (3, n))
    b = rng.integers(2, 9, n)                                      # shapes 2 .. 8: the window is 4, 5, 6
    b[:B] = [4, 5, 6]
    keys = morton_keys(x, y, z, b, depth)
    keys = np.concatenate([keys, keys[:50],                        # duplicates
                           morton_keys([8, 3], [1, 9], [2, 2], [5, 5], depth + 1)])       # x or y >= R: a deeper key
    occ = np.zeros((B, R, R, R), bool)
    m = (b >= b0) & (b < b0 + B)
    occ[b[m] - b0, x[m], y[m], z[m]] = True
    for weld in (0, 1):
        VmRun(B, depth, weld, keys_fill(keys, b0, B, depth), gaps=weld).check(occ)
    # fewer keys into the same workspace: the mask is cleared first, no stale bit reaches the count
    ws = workspace(lib().ofx_voxmesh_ws_bytes(B, depth, 0))
    counts = Guarded(B, I64, cols=2)
    keys_fill(keys, b0, B, depth)(ws)
    few = morton_keys([1], [2], [3], [5], depth)
    keys_fill(few, b0, B, depth)(ws)
    _call('ofx_voxmesh_count', B, depth, 0, ws.ptr, counts.ptr)
    assert counts.get().tolist() == [[0, 0], [6, 0], [0, 0]]
    _call('ofx_voxmesh_mask_keys', None, 0, b0, B, depth, ws.ptr)  # n == 0: NULL keys are fine, everything is cleared
    _call('ofx_voxmesh_count', B, depth, 0, ws.ptr, counts.ptr)
    assert not counts.get().any() and ws.bands_intact()


def test_voxmesh_mask_dense_threshold_and_non_finite_values():
    depth, R, thr = 2, 4, np.float32(0.4)
    g = np.full((2, R, R, R), thr, np.float32)                     # equal to the threshold: empty
    g[0, 1, 1, 1] = 1.0
    g[0, 1, 1, 2] = np.nan                                         # its +z neighbour: empty, the face is exposed
    g[0, 1, 2, 1] = np.inf
    g[0, 2, 1, 1] = -np.inf
    g[0, 0, 0, 0] = np.nextafter(thr, np.float32(1))   # one ulp above: occupied, three faces on the boundary
    g[1, R - 1, R - 1, R - 1] = 2.0
    occ = np.zeros((2, R, R, R), bool)
    occ[0, 1, 1, 1] = occ[0, 0, 0, 0] = occ[1, R - 1, R - 1, R - 1] = True
    assert np.array_equal(VO.occupancy(g, thr), occ)
    for weld in (0, 1):
        run = VmRun(2, depth, weld, dense_fill(g, float(thr)), gaps=weld)
        want = [VO.mesh(g[b], thr, weld=bool(weld)) for b in range(2)]
        run.check(None, want=want)
        assert run.c[:, 0].tolist() == [12, 6]


def test_voxmesh_largest_batch_of_depth_1():
    """65 535 grids of 2^3 cells (2 MB): the shape index fills the second grid dimension of the dense fill."""
    rng = np.random.default_rng(1)
    g = (rng.random((MAX_BATCH, 2, 2, 2)) < 0.5).astype(np.float32)
    run = VmRun(MAX_BATCH, 1, 1, dense_fill(g, 0.5), gaps=1)
    occ = g > 0.5
    pad = np.zeros((MAX_BATCH, 4, 4, 4), bool)
    pad[:, 1:3, 1:3, 1:3] = occ
    quads = sum((occ & ~pad[:, 1 + d[0]:3 + d[0], 1 + d[1]:3 + d[1], 1 + d[2]:3 + d[2]]).sum((1, 2, 3)) for d in VO.DIRS)
    assert np.array_equal(run.c[:, 0], quads)
    sample = np.concatenate([[0, MAX_BATCH - 1], rng.integers(0, MAX_BATCH, 200)])
    run.check(occ, shapes=sample.tolist())
    assert lib().ofx_voxmesh_ws_bytes(MAX_BATCH + 1, 1, 1) == 0
    t = up(g[:1], F32)
    _refused('ofx_voxmesh_mask_dense', t.data_ptr(), MAX_BATCH + 1, 1, 0.5, run.ws.ptr)


def test_voxmesh_ws_bytes_limits():
    ws = lib().ofx_voxmesh_ws_bytes
    for weld in (0, 1):
        assert ws(1, 0, weld) == 0 and ws(1, 9, weld) == 0 and ws(0, 3, weld) == 0 and ws(-1, 3, weld) == 0
        for depth in range(1, 9):
            top = min(MAX_BATCH, INT32_MAX // (24 * 8 ** depth))
            assert top >= 1 and ws(top, depth, weld) > 0 and ws(top + 1, depth, weld) == 0
        assert ws(1, 8, weld) > 0
    assert ws(3, 4, 1) > ws(3, 4, 0)
    assert MAX_BATCH <= max_grid_dim_y()


def test_voxmesh_refusals():
    depth, B = 2, 2
    ws = workspace(lib().ofx_voxmesh_ws_bytes(B, depth, 1))
    counts, verts, faces = Guarded(B, I64, cols=2), Guarded(64, F32, cols=3), Guarded(64, I32, cols=3)
    occ, keys, offs = up(np.ones((B, 4, 4, 4)), F32), up(np.zeros(4), I64), up(np.zeros(2 * B), I64)
    for a in ([None, 4, 0, B, depth, ws.ptr], [keys.data_ptr(), -1, 0, B, depth, ws.ptr],
              [keys.data_ptr(), 4, -1, B, depth, ws.ptr], [keys.data_ptr(), 4, 0, B, depth, None],
              [keys.data_ptr(), 4, 0, 0, depth, ws.ptr], [keys.data_ptr(), 4, 0, B, 0, ws.ptr],
              [keys.data_ptr(), 4, 0, B, 9, ws.ptr]):
        _refused('ofx_voxmesh_mask_keys', *a)
    for a in ([None, B, depth, 0.4, ws.ptr], [occ.data_ptr(), B, depth, 0.4, None],
              [occ.data_ptr(), B, depth, float('nan'), ws.ptr], [occ.data_ptr(), 0, depth, 0.4, ws.ptr],
              [occ.data_ptr(), B, 0, 0.4, ws.ptr], [occ.data_ptr(), B, 9, 0.4, ws.ptr]):
        _refused('ofx_voxmesh_mask_dense', *a)
    for weld in (0, 1):
        for a in ([B, depth, weld, None, counts.ptr], [B, depth, weld, ws.ptr, None], [0, depth, weld, ws.ptr, counts.ptr],
                  [B, 0, weld, ws.ptr, counts.ptr], [B, 9, weld, ws.ptr, counts.ptr]):
            _refused('ofx_voxmesh_count', *a)
        good = [B, depth, weld, ws.ptr, offs.data_ptr(), offs.data_ptr(), verts.ptr, faces.ptr]
        for i in (3, 4, 5, 6, 7):
            a = list(good)
            a[i] = None
            _refused('ofx_voxmesh_emit', *a)
        _refused('ofx_voxmesh_emit', 0, *good[1:])
        _refused('ofx_voxmesh_emit', B, 9, *good[2:])
    settled(ws, counts, verts, faces)
