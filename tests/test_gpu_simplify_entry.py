"""The simplification kernels (csrc/ofx_simplify.hip) one entry point at a time through the C ABI, against
tests/simplify_oracle.py.  Every output is prefilled with a sentinel and sits, like the workspace (sized exactly by
ofx_simplify_ws_bytes), between sentinel bands; the offsets of the extract call leave gaps, which must keep the
sentinel; a second pass over the same workspace must give the same bytes.

    entry point             cases                                                             refusals / status
    ofx_simplify_stages     5; stages 1 .. 4 of the cluster call                              stages 0 and 6: OFX_EINVAL
    ofx_simplify_ws_bytes   --                                                                0: V = 2^31 - 1,
                                                                                              F = (2^31 - 1) / 3 + 1, batch 0
    ofx_simplify_cluster    300 tiny shapes and a 2000-vertex sphere in one batch and         NULLs, cells, cell_size, reg
                            alone, `cells` and `cell_size`; boxes of extent zero, flat        out of range; status[0] for
                            and one ulp wide; cells = 1 and 1024; a cell_size that needs      offsets and indices (column
                            1023 / 1024 cells; a NaN / infinite vertex, used or not           5), status[1] bit 0 (column
                                                                                              6) and bit 1 (column 7)
    ofx_simplify_extract    the same; new offsets with gaps                                   NULLs; status[0] on entry

Counts and faces are compared exactly, vertices within one fp32 ulp at the mesh's largest coordinate (the bound
test_gpu_simplify.py derives); "alone" against "in a batch" bit for bit.
"""
import numpy as np
import pytest
import torch

import mesh_entry_util as U
import simplify_oracle as S
from mesh_entry_util import INT32_MAX, Guarded, _call, _refused, lib, settled, up, workspace

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

F32, I32, I64 = torch.float32, torch.int32, torch.int64
REG = 1e-3


def expected(meshes, **kw):
    """counts rows [B, 8] and the outputs of every shape, from the oracle."""
    rows, outs = [], []
    for v, f in meshes:
        wv, wf = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
        if len(v) == 0:
            rows.append([0] * 8)
        elif len(f) == 0:                                              # vertices without faces still occupy cells
            rows.append([len(np.unique(S.grid(v, **kw)[2], axis=0))] + [0] * 7)
        else:
            wv, wf, st = S.simplify(v, f, reg=REG, **kw)
            rows.append([st['clusters'], len(wv), len(wf), st['faces_collapsed'], st['faces_duplicate'], 0, 0, 0])
            assert st['clusters_unused'] == st['clusters'] - len(wv)
        outs.append((wv, wf))
    return np.array(rows, np.int64), outs


class SpRun:
    def __init__(self, meshes=None, raw=None, cells=None, cell_size=None, reg=REG, stages=None):
        self.meshes = meshes
        self.v, self.f, self.voff, self.toff = U.cat(meshes) if raw is None else raw
        self.B, self.V, self.F = len(self.voff) - 1, len(self.v), len(self.f)
        self.kw = dict(cells=cells) if cells is not None else dict(cell_size=cell_size)
        self.mode = (int(cells) if cells is not None else 0, float(cell_size) if cell_size is not None else 0.0,
                     float(reg), lib().ofx_simplify_stages() if stages is None else stages)
        nbytes = lib().ofx_simplify_ws_bytes(self.V, self.F, self.B)
        assert nbytes > 0
        self.ws = workspace(nbytes)
        self.dv, self.df = up(self.v, F32), up(self.f, I32)
        self.dvo, self.dto = up(self.voff, I64), up(self.toff, I64)
        self.counts, self.status = Guarded(self.B, I64, cols=8), Guarded(2, I32)
        self.sizes = (self.B, self.V, self.F)

    def cluster_args(self):
        return [self.dv.data_ptr(), self.df.data_ptr(), self.dvo.data_ptr(), self.dto.data_ptr(), *self.sizes,
                *self.mode, self.counts.ptr, self.ws.ptr, self.status.ptr]

    def cluster(self):
        _call('ofx_simplify_cluster', *self.cluster_args())
        return self

    def extract_args(self):
        return [self.df.data_ptr(), self.dvo.data_ptr(), self.dto.data_ptr(), *self.sizes, self.new.data_ptr(),
                self.new.data_ptr() + 8 * self.B, self.out_v.ptr, self.out_f.ptr, self.ws.ptr, self.status.ptr]

    def extract(self, gaps=None):
        c = self.c = self.counts.get()
        kv, kf = c[:, 1], c[:, 2]
        if gaps is None:
            self.nvo, nv, self.nto, nt = np.cumsum(kv) - kv, int(kv.sum()), np.cumsum(kf) - kf, int(kf.sum())
        else:
            rng = np.random.default_rng(gaps)
            self.nvo, nv = U.gapped(kv, rng)
            self.nto, nt = U.gapped(kf, rng)
        self.out_v, self.out_f = Guarded(max(nv, 1), F32, cols=3), Guarded(max(nt, 1), I32, cols=3)
        self.new = up(np.stack([self.nvo, self.nto]), I64)
        _call('ofx_simplify_extract', *self.extract_args())
        self.host = None
        return self

    def shape(self, b):
        if self.host is None:                                          # one readback for all shapes
            self.host = self.out_v.get(), self.out_f.get()
        ov, of = self.host
        return ov[self.nvo[b]:self.nvo[b] + self.c[b, 1]], of[self.nto[b]:self.nto[b] + self.c[b, 2]]

    def guards(self):
        return self.ws.bands_intact() and self.counts.bands_intact() and self.status.bands_intact() and \
            self.out_v.bands_intact() and self.out_f.bands_intact()

    def check(self, gaps=None, skip=()):
        """cluster + extract against the oracle (shapes in `skip` excepted), the gaps, and a second pass."""
        rows, outs = expected([m if b not in skip else (m[0][:0], m[1][:0]) for b, m in enumerate(self.meshes)],
                              **self.kw)
        self.cluster().extract(gaps)
        keep = [b for b in range(self.B) if b not in skip]
        assert self.status.get().tolist()[0] == 0
        assert np.array_equal(self.c[keep], rows[keep])
        for b in keep:
            gv, gf = self.shape(b)
            wv, wf = outs[b]
            assert np.array_equal(gf, wf), b
            if len(wv):
                tol = np.spacing(np.float32(np.abs(self.meshes[b][0]).max()))
                assert np.abs(gv.astype(np.float64) - wv.astype(np.float64)).max() <= tol, b
        vm, tm = U.rows_of(self.nvo, self.c[:, 1]), U.rows_of(self.nto, self.c[:, 2])
        vrows, trows = np.ones(self.out_v.n // 3, bool), np.ones(self.out_f.n // 3, bool)
        vrows[:len(vm)] = ~vm
        trows[:len(tm)] = ~tm
        assert self.out_v.is_sentinel(vrows) and self.out_f.is_sentinel(trows) and self.guards()
        first = (self.counts.raw(), self.status.raw(), self.out_v.raw(), self.out_f.raw())
        self.counts.reset()
        self.status.reset()
        self.cluster().extract(gaps)
        again = (self.counts.raw(), self.status.raw(), self.out_v.raw(), self.out_f.raw())
        assert all(np.array_equal(a, b) for a, b in zip(first, again)) and self.guards()
        return self


def same_alone(run, b, **kw):
    """Shape b of a batch run, run alone: the same counts and the same bytes."""
    one = SpRun([run.meshes[b]], **kw).cluster().extract()
    assert np.array_equal(one.c[0], run.c[b]), b
    gv, gf = run.shape(b)
    ov, of = one.shape(0)
    assert np.array_equal(ov.view(np.int32), gv.view(np.int32)) and np.array_equal(of, gf), b
    assert one.status.get().tolist() == run.status.get().tolist() == [0, 0] and one.guards()


# ------------------------------------------------------------------------------------------------ many tiny shapes
@pytest.mark.parametrize('kw', [dict(cells=3), dict(cell_size=0.375)], ids=['cells', 'cell_size'])
def test_300_tiny_shapes_and_a_sphere_in_one_batch_and_alone(kw):
    kinds, meshes = U.tiny_batch()
    meshes = meshes + [U.uv_sphere()]
    assert len(meshes) == 301 and len(meshes[-1][0]) == 2000
    run = SpRun(meshes, **kw).check(gaps=301)
    assert run.status.get().tolist() == [0, 0]
    assert run.c[-1, 2] > 0 and (run.c[:, 0] > 0).sum() > 200
    alone = 0
    for b, (v, f) in enumerate(meshes):
        if len(v) and len(f):
            same_alone(run, b, **kw)
            alone += 1
    assert alone >= 100


# ------------------------------------------------------------------------------------------------ degenerate boxes
def degenerate_meshes():
    one = np.float32(1.0)
    point = np.tile(np.array([[0.25, -3.0, 7.5]], np.float32), (5, 1))
    line = np.stack([np.arange(6, dtype=np.float32) * np.float32(0.3), np.full(6, 2, np.float32),
                     np.full(6, -1, np.float32)], 1)
    thin = np.array([[one, 0, 0], [np.nextafter(one, np.float32(2)), 0, 0], [one, 0, 0],
                     [np.nextafter(one, np.float32(2)), 0, 0]], np.float32)
    strip = np.array([[0, 1, 2], [1, 2, 3], [2, 3, 4]], np.int32)
    return [(point, strip), (line, np.array([[0, 1, 2], [1, 3, 5], [0, 2, 4], [5, 4, 3]], np.int32)),
            (thin, np.array([[0, 1, 2], [1, 2, 3]], np.int32)), U.uv_sphere(8, 9)]


@pytest.mark.parametrize('kw', [dict(cells=3), dict(cells=1024), dict(cell_size=0.25)], ids=['cells3', 'cells1024', 'size'])
def test_degenerate_boxes(kw):
    run = SpRun(degenerate_meshes(), **kw).check(gaps=1)
    assert run.status.get().tolist() == [0, 0]
    assert run.c[0].tolist() == [1, 0, 0, 3, 0, 0, 0, 0]               # side == 0: one cluster, every face collapses
    assert run.c[2, 2] == 0                                            # two clusters at the most: every face collapses
    for b in range(4):
        same_alone(run, b, **kw)


# ------------------------------------------------------------------------------------------------ grid limits
@pytest.mark.parametrize('cells', [1, 2, 1023, 1024])
def test_cells_limits(cells):
    """cells = 1024: the vertices on the box's upper faces are clamped into cell 1023, all ten key bits set."""
    sphere = U.uv_sphere(10, 12)
    detail = {}
    S.simplify(*sphere, cells=cells, detail=detail)
    if cells > 2:
        assert detail['cell'].max() == cells - 1
    run = SpRun([sphere, U.tiny_shape('pair', np.random.default_rng(2))], cells=cells).check(gaps=cells)
    assert run.status.get().tolist() == [0, 0]
    if cells == 1:
        assert run.c[:, :3].tolist() == [[1, 0, 0], [1, 0, 0]]


def test_cell_size_that_needs_1023_or_1024_cells():
    mesh = (U.TETRA_V.copy(), U.TETRA_F.copy())                        # extent exactly 1 along every axis
    other = U.uv_sphere(6, 7, r=0.01)
    over, fits = U.OVERFLOW_CELL_SIZES
    run = SpRun([other, mesh, other], cell_size=fits).check(gaps=2)
    assert run.status.get().tolist() == [0, 0] and not run.c[:, 6].any()
    run = SpRun([other, mesh, other], cell_size=over).check(gaps=2, skip=(1,))
    assert run.status.get().tolist() == [0, 1] and run.c[:, 6].tolist() == [0, 1, 0] and not run.c[:, 7].any()
    with pytest.raises(ValueError, match='grid overflow'):
        S.simplify(*mesh, cell_size=over)
    for b in (0, 2):                                                   # the neighbours of the flagged shape
        one = SpRun([other], cell_size=over).cluster().extract()
        assert np.array_equal(one.c[0], run.c[b])
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(one.shape(0), run.shape(b)))


# ------------------------------------------------------------------------------------------------ stages
def test_stages():
    full = lib().ofx_simplify_stages()
    assert full == 5
    meshes = [U.uv_sphere(10, 12), U.tiny_shape('unused', np.random.default_rng(3))]
    for stages in range(1, full):
        run = SpRun(meshes, cells=4, stages=stages).cluster()
        assert run.status.get().tolist() == [0, 0] and not run.counts.get().any()      # columns 0-4 wait for the face pass
        assert run.ws.bands_intact()
    bad = (meshes[1][0].copy(), meshes[1][1])
    bad[0][0, 1] = np.nan
    for stages in range(1, full + 1):                                  # the flags are complete from stage 1 on
        run = SpRun([meshes[0], bad, (U.TETRA_V * np.float32(300), U.TETRA_F)], cell_size=0.25, stages=stages).cluster()
        assert run.status.get().tolist() == [0, 3]
        assert run.counts.get()[:, 5:].tolist() == [[0, 0, 0], [0, 0, 1], [0, 1, 0]] and run.ws.bands_intact()
    run = SpRun(meshes, cells=4)
    for stages in (0, -1, full + 1):
        a = run.cluster_args()
        a[10] = stages
        _refused('ofx_simplify_cluster', *a)
    settled(run.ws, run.counts, run.status)


# ------------------------------------------------------------------------------------------------ status
def _pair_batch():
    return [U.tiny_shape('tetra', np.random.default_rng(0)), U.tiny_shape('pair', np.random.default_rng(1))]


@pytest.mark.parametrize('case', ['vert_off0', 'tri_off0', 'descending_vert', 'descending_tri', 'last_vert',
                                  'last_tri'])
def test_status_inconsistent_offsets(case):
    v, f, voff, toff = U.cat(_pair_batch())
    voff, toff = voff.copy(), toff.copy()
    if case == 'vert_off0':
        voff[0] = 1
    elif case == 'tri_off0':
        toff[0] = 1
    elif case == 'descending_vert':
        voff[1] = voff[2] + 1
    elif case == 'descending_tri':
        toff[1] = toff[2] + 1
    elif case == 'last_vert':
        voff[2] -= 1
    else:
        toff[2] -= 1
    run = SpRun(raw=(v, f, voff, toff), cells=3).cluster()
    assert run.status.get().tolist() == [2, 0] and not run.counts.get().any()     # nobody followed the tables
    run.c = np.zeros((2, 8), np.int64)
    run.counts.set(np.array([[1, 4, 4, 0, 0, 0, 0, 0]] * 2))           # whatever the caller believes: nothing is written
    run.extract(gaps=1)
    torch.cuda.synchronize()
    assert run.out_v.untouched() and run.out_f.untouched() and run.guards()


def test_status_bad_index_and_status_on_entry():
    v, f, voff, toff = U.cat(_pair_batch())
    f = f.copy()
    f[2, 1] = 4                                                        # shape 0 has vertices 0 .. 3; 4 exists in the batch
    run = SpRun(raw=(v, f, voff, toff), cells=3).cluster()
    assert run.status.get().tolist() == [1, 0]
    assert run.counts.get().tolist() == [[0, 0, 0, 0, 0, 1, 0, 0], [0] * 8]
    f[2, 1], f[5, 0] = 3, -1                                           # the other shape, a negative index
    run = SpRun(raw=(v, f, voff, toff), cell_size=0.5).cluster()
    assert run.status.get().tolist() == [1, 0]
    assert run.counts.get().tolist() == [[0] * 8, [0, 0, 0, 0, 0, 1, 0, 0]]
    # a good run, then status[0] set by the caller: extract leaves its outputs alone
    f[5, 0] = 0
    run = SpRun(raw=(v, f, voff, toff), cells=3).cluster()
    assert run.status.get().tolist() == [0, 0] and run.counts.get()[:, 5:].tolist() == [[0, 0, 0]] * 2
    run.status.set([1, 0])
    run.extract(gaps=3)
    torch.cuda.synchronize()
    assert run.out_v.untouched() and run.out_f.untouched() and run.guards()
    run.status.set([0, 0])
    run.extract(gaps=3)
    assert not run.out_v.untouched()


# ------------------------------------------------------------------------------------------------ non-finite vertices
@pytest.mark.parametrize('kw', [dict(cells=8), dict(cell_size=0.125)], ids=['cells', 'cell_size'])
@pytest.mark.parametrize('where', ['used', 'unused'])
@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_non_finite_vertex_is_refused_for_its_shape_only(bad, where, kw):
    """On the parent commit the `cells` cases came back with status (0, 0) and the shape collapsed to one cluster."""
    good0, good2 = U.uv_sphere(10, 12), U.tiny_shape('pair', np.random.default_rng(4))
    v, f = U.tiny_shape('unused', np.random.default_rng(5))            # vertices 0, 1 and 6 are used by no face
    assert not np.isin([0, 1, 6], f).any()
    v = v.copy()
    v[3 if where == 'used' else 6, 1] = bad
    assert S.nonfinite(v) and not S.nonfinite(good0[0])
    with pytest.raises(ValueError, match='non-finite'):
        S.simplify(v, f, **kw)
    run = SpRun([good0, (v, f), good2], **kw).check(gaps=7, skip=(1,))
    assert run.status.get().tolist() == [0, 2]
    assert run.c[:, 7].tolist() == [0, 1, 0] and not run.c[:, 5:7].any()
    assert run.c[1, :3].tolist() == [1, 0, 0]                          # left as one cluster, nothing kept
    for b in (0, 2):
        one = SpRun([run.meshes[b]], **kw).cluster().extract()
        assert np.array_equal(one.c[0], run.c[b]) and one.status.get().tolist() == [0, 0]
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(one.shape(0), run.shape(b)))
    from octfusion_amd import simplify
    dev = lambda m: (torch.from_numpy(np.ascontiguousarray(m[0])).to(U.dev()), torch.from_numpy(m[1]).to(U.dev()))
    with pytest.raises(ValueError, match=r'simplify: shape 1 has a non-finite vertex'):
        simplify.simplify([dev(good0), dev((v, f)), dev(good2)], **kw)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    ws = lib().ofx_simplify_ws_bytes
    assert ws(INT32_MAX, 10, 1) == 0 and ws(10, INT32_MAX // 3 + 1, 1) == 0 and ws(10, 10, 0) == 0
    assert ws(0, 10, 1) == 0 and ws(10, 0, 1) == 0 and ws(10, 10, -1) == 0 and ws(10, 10, 1) > 0
    run = SpRun(_pair_batch(), cells=3)
    run.out_v, run.out_f, run.new = Guarded(16, F32, cols=3), Guarded(16, I32, cols=3), up(np.zeros(4), I64)
    good = run.cluster_args()
    nan, inf = float('nan'), float('inf')
    variants = [(7, -1), (7, 1025), (9, 0.0), (9, 1.5), (9, nan), (9, -0.5), (4, 0), (5, 0), (6, 0), (5, INT32_MAX),
                (6, INT32_MAX // 3 + 1)] + [(i, None) for i in (0, 1, 2, 3, 11, 12, 13)]
    for i, bad in variants:
        a = list(good)
        a[i] = bad
        _refused('ofx_simplify_cluster', *a)
    for size in (0.0, -1.0, nan, inf, -inf):                           # cells == 0 needs a finite cell_size > 0
        a = list(good)
        a[7], a[8] = 0, size
        _refused('ofx_simplify_cluster', *a)
    good = run.extract_args()
    for i, bad in [(3, 0), (4, 0), (5, 0), (4, INT32_MAX)] + [(i, None) for i in (0, 1, 2, 6, 7, 8, 9, 10, 11)]:
        a = list(good)
        a[i] = bad
        _refused('ofx_simplify_extract', *a)
    settled(run.ws, run.counts, run.status, run.out_v, run.out_f)
