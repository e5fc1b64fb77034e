"""The component kernels (csrc/ofx_mesh_cc.hip) one entry point at a time through the C ABI, against tests/cc_oracle.py
-- bit for bit.  Every output is prefilled with a sentinel and sits, like the workspace (sized exactly by
ofx_mesh_cc_ws_bytes), between sentinel bands; a second pass over the same workspace must give the same bytes.

    entry point            cases                                                              refusals / status
    ofx_mesh_cc_ws_bytes   --                                                                 0: V, F, batch of 0, 2^31
    ofx_mesh_cc_label      300 tiny shapes (empty ones, unused vertices) in one batch and     NULLs; status[1] bit 1 for
                           alone; a 20 000-face fan, a comb, a reversed strip                 every inconsistent offset
                                                                                              table, bit 0 for an index
                                                                                              == the shape's vertex count
    ofx_mesh_cc_table      the same; comp_of_vert == NULL writes comp_off only                NULLs; status[1] on entry
    ofx_mesh_cc_stats      the same; -0.0 / +0.0, denormals, +-inf in a box; n_comp below     NULLs, n_comp < 0; status[1]
                           the true count; n_comp == 0                                        on entry
    ofx_mesh_cc_select     the same; extents that tie in fp32 and differ in fp64, a tie on    NULLs; status[1] on entry
                           different axes, shapes without faces; keep_counts column 2
    ofx_mesh_cc_extract    the same; new offsets with gaps                                    NULLs; status[1] on entry
"""
import numpy as np
import pytest
import torch

import cc_oracle as CO
import mesh_entry_util as U
from mesh_entry_util import Arena, Guarded, _call, _refused, lib, settled, up, workspace

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

F32, I32, I64 = torch.float32, torch.int32, torch.int64


def expected(meshes):
    """Everything the five entries write for a batch, from the oracle, shape by shape."""
    e = dict(label=[], cov=[], comp_off=[0], rows=[], winner=[], keep=[], out_v=[], out_f=[])
    for v, f in meshes:
        tab = CO.table(v, f)
        cv, K, nv = tab['comp_of_vert'], len(tab['n_verts']), len(v)
        first = np.full(K, nv, np.int64)
        np.minimum.at(first, cv[cv >= 0], np.nonzero(cv >= 0)[0])
        lab = np.arange(nv, dtype=np.int64)
        lab[cv >= 0] = first[cv[cv >= 0]]
        e['label'].append(lab)
        e['cov'].append(cv)
        e['comp_off'].append(e['comp_off'][-1] + K)
        e['rows'].append(np.concatenate([tab['bbox_min'].reshape(K, 3).view(np.int32).astype(np.int64),
                                         tab['bbox_max'].reshape(K, 3).view(np.int32).astype(np.int64),
                                         tab['n_verts'][:, None], tab['n_faces'][:, None]], 1))
        w = CO.select(tab)
        if w < 0:
            e['winner'].append(-1)
            e['keep'].append((0, 0, 0))
            e['out_v'].append(np.zeros((0, 3), np.float32))
            e['out_f'].append(np.zeros((0, 3), np.int32))
        else:
            ov, of = CO.extract(v, f, w, tab)
            e['winner'].append(int(first[w]))
            e['keep'].append((len(ov), len(of), K))
            e['out_v'].append(ov)
            e['out_f'].append(of)
    for k in ('label', 'cov', 'rows'):
        e[k] = np.concatenate(e[k])
    e['comp_off'], e['winner'], e['keep'] = np.array(e['comp_off']), np.array(e['winner']), np.array(e['keep'])
    return e


class CcRun:
    def __init__(self, meshes=None, raw=None):
        self.v, self.f, self.voff, self.toff = U.cat(meshes) if raw is None else raw
        self.B, self.V, self.F = len(self.voff) - 1, len(self.v), len(self.f)
        nbytes = lib().ofx_mesh_cc_ws_bytes(self.V, self.F, self.B)
        assert nbytes > 0
        self.ws = workspace(nbytes)
        self.dv, self.df = up(self.v, F32), up(self.f, I32)
        self.dvo, self.dto = up(self.voff, I64), up(self.toff, I64)
        self.ints = Arena([self.V, self.V, self.B + 1, self.B])          # label, comp_of_vert, comp_off, winner
        self.status = Guarded(2, I32)
        self.keep = Guarded(3 * self.B, I64)
        self.sizes = (self.B, self.V, self.F)

    def mesh_args(self, verts=False):
        a = [self.df.data_ptr(), self.dvo.data_ptr(), self.dto.data_ptr()]
        return ([self.dv.data_ptr()] if verts else []) + a

    def label(self):
        _call('ofx_mesh_cc_label', *self.mesh_args(), *self.sizes, self.ints.ptr(0), self.ws.ptr, self.status.ptr)
        return self

    def table(self, cov=True):
        a = self.mesh_args()
        _call('ofx_mesh_cc_table', a[0], self.ints.ptr(0), a[1], a[2], *self.sizes, self.ints.ptr(1) if cov else None,
              self.ints.ptr(2), self.ws.ptr, self.status.ptr)
        return self

    def stats(self, n_comp, rows=None):
        self.tab = Guarded(max(n_comp if rows is None else rows, 1), I32, cols=8)
        a = self.mesh_args(True)
        _call('ofx_mesh_cc_stats', a[0], a[1], self.ints.ptr(0), a[2], a[3], *self.sizes, n_comp, self.tab.ptr,
              self.ws.ptr, self.status.ptr)
        return self

    def select(self):
        a = self.mesh_args(True)
        _call('ofx_mesh_cc_select', a[0], a[1], self.ints.ptr(0), a[2], a[3], *self.sizes, self.ints.ptr(3),
              self.keep.ptr, self.ws.ptr, self.status.ptr)
        return self

    def extract(self, keep, gaps=None):
        kv, kf = keep[:, 0], keep[:, 1]
        if gaps is None:
            self.nvo, nv, self.nto, nt = np.cumsum(kv) - kv, int(kv.sum()), np.cumsum(kf) - kf, int(kf.sum())
        else:
            rng = np.random.default_rng(gaps)
            self.nvo, nv = U.gapped(kv, rng)
            self.nto, nt = U.gapped(kf, rng)
        self.out_v, self.out_f = Guarded(max(nv, 1), F32, cols=3), Guarded(max(nt, 1), I32, cols=3)
        self.new = up(np.stack([self.nvo, self.nto]), I64)
        a = self.mesh_args(True)
        _call('ofx_mesh_cc_extract', *a, *self.sizes, self.new.data_ptr(), self.new.data_ptr() + 8 * self.B,
              self.out_v.ptr, self.out_f.ptr, self.ws.ptr, self.status.ptr)
        return self

    def guards(self):
        return self.ws.bands_intact() and self.ints.guards_intact() and self.status.bands_intact() and \
            self.keep.bands_intact()

    def everything(self, want, gaps=None):
        """All five entries against `want` (expected(...)); returns the bytes of every output."""
        B = self.B
        self.label().table()
        assert self.status.get().tolist() == [0, 0]
        assert np.array_equal(self.ints.get(0), want['label'])
        assert np.array_equal(self.ints.get(1), want['cov'])
        assert np.array_equal(self.ints.get(2), want['comp_off'])
        K = int(want['comp_off'][-1])
        self.stats(K)
        if K:
            assert np.array_equal(self.tab.get(), want['rows'])
        else:
            assert self.tab.untouched()
        self.select()
        keep = self.keep.get().reshape(3, B).T                       # [B, 3]: kept vertices, kept faces, components
        assert np.array_equal(self.ints.get(3), want['winner'])
        assert np.array_equal(keep, want['keep'])
        self.extract(keep, gaps)
        ov, of = self.out_v.get(), self.out_f.get()
        for b in range(B):
            nv, nf = keep[b, 0], keep[b, 1]
            assert np.array_equal(ov[self.nvo[b]:self.nvo[b] + nv].view(np.int32), want['out_v'][b].view(np.int32)), b
            assert np.array_equal(of[self.nto[b]:self.nto[b] + nf], want['out_f'][b]), b
        vm, tm = U.rows_of(self.nvo, keep[:, 0]), U.rows_of(self.nto, keep[:, 1])
        vrows, trows = np.ones(len(ov), bool), np.ones(len(of), bool)
        vrows[:len(vm)] = ~vm
        trows[:len(tm)] = ~tm
        assert self.out_v.is_sentinel(vrows) and self.out_f.is_sentinel(trows)       # the gaps, and the tail
        assert self.status.get().tolist() == [0, 0] and self.guards()
        return [self.ints.get(i).tobytes() for i in range(4)] + [self.tab.raw().tobytes(), self.keep.raw().tobytes(),
                                                                 self.out_v.raw().tobytes(), self.out_f.raw().tobytes()]


def check_twice(meshes, gaps=None):
    want = expected(meshes)
    run = CcRun(meshes)
    first = run.everything(want, gaps)
    run.ints.buf.fill_(U.SENT[I32])
    run.keep.reset()
    assert first == run.everything(want, gaps)                       # the same workspace again: the same bytes
    return run, want


# ------------------------------------------------------------------------------------------------ many tiny shapes
def test_300_tiny_shapes_in_one_batch_and_alone():
    kinds, meshes = U.tiny_batch()
    assert len(meshes) == 300 and set(kinds) == set(U.KINDS)
    run, want = check_twice(meshes, gaps=300)
    label, cov, rows = run.ints.get(0), run.ints.get(1), run.tab.get()
    keep, winner = run.keep.get().reshape(3, 300).T, run.ints.get(3)
    ov, of = run.out_v.get(), run.out_f.get()
    alone = 0
    for b, (v, f) in enumerate(meshes):
        if len(v) == 0 or len(f) == 0:
            assert winner[b] == -1 and keep[b].tolist() == [0, 0, 0]
            continue
        one = CcRun([(v, f)])
        one.label().table()
        k0, k1 = want['comp_off'][b], want['comp_off'][b + 1]
        one.stats(int(k1 - k0)).select()
        k = one.keep.get().reshape(3, 1).T
        one.extract(k)
        v0, v1 = run.voff[b], run.voff[b + 1]
        assert np.array_equal(one.ints.get(0), label[v0:v1]) and np.array_equal(one.ints.get(1), cov[v0:v1])
        assert one.ints.get(2).tolist() == [0, k1 - k0] and np.array_equal(one.tab.get(), rows[k0:k1])
        assert one.ints.get(3)[0] == winner[b] and np.array_equal(k[0], keep[b])
        assert np.array_equal(one.out_v.get().view(np.int32), ov[run.nvo[b]:run.nvo[b] + keep[b, 0]].view(np.int32))
        assert np.array_equal(one.out_f.get(), of[run.nto[b]:run.nto[b] + keep[b, 1]])
        assert one.status.get().tolist() == [0, 0] and one.guards()
        alone += 1
    assert alone >= 100


# ------------------------------------------------------------------------------------------------ topologies
def test_fan_comb_and_reversed_strip():
    meshes = [U.fan(20000), U.comb(40, 60), U.reversed_strip(5000), CO.strip(3000, seed=4, cut=1500)]
    run, want = check_twice(meshes, gaps=2)
    assert np.diff(want['comp_off']).tolist() == [1, 1, 1, 2]
    assert not run.ints.get(0)[:20002].any()                         # every vertex of the fan under the hub


# ------------------------------------------------------------------------------------------------ optional output
def test_table_without_comp_of_vert():
    _, meshes = U.tiny_batch(40, seed=9)
    want = expected(meshes)
    run = CcRun(meshes).label().table(cov=False)
    assert np.array_equal(run.ints.get(2), want['comp_off'])
    assert bool((run.ints.view(1) == U.SENT[I32]).all()) and run.guards()


# ------------------------------------------------------------------------------------------------ stats
def special_box_mesh():
    tiny = np.float32(1e-45)
    v = np.array([[0.0, tiny, np.inf], [-0.0, -tiny, -np.inf], [0.0, 0.0, 1.0], [-0.0, tiny, 2.0],     # component 0
                  [5.0, -0.0, -0.0], [6.0, -0.0, -0.0], [7.0, -0.0, -0.0],                               # component 1
                  [9.0, 9.0, 9.0]], np.float32)                                                          # unused
    f = np.array([[1, 0, 2], [2, 3, 0], [4, 5, 6]], np.int32)
    return v, f


def test_stats_signed_zeros_denormals_infinities_and_fewer_rows():
    v, f = special_box_mesh()
    sphere = U.uv_sphere(10, 12)
    meshes = [sphere, (v, f), (v[::-1].copy(), (7 - f).astype(np.int32))]
    want = expected(meshes)
    run = CcRun(meshes).label().table()
    K = int(want['comp_off'][-1])
    assert K == 5
    run.stats(K)
    rows = run.tab.get()
    assert np.array_equal(rows, want['rows'])
    bits = lambda x: int(np.float32(x).view(np.int32))
    for r in (rows[1], rows[4]):                                     # component 0 of the special mesh, both orders
        assert r[0] == bits(-0.0) and r[3] == bits(0.0)              # -0.0 is the min, +0.0 the max
        assert r[1] == bits(-1e-45) and r[4] == bits(1e-45) and r[2] == bits(-np.inf) and r[5] == bits(np.inf)
        assert r[6] == 4 and r[7] == 2
    for r in (rows[2], rows[3]):
        assert r[1] == r[2] == r[4] == r[5] == bits(-0.0) and r[6] == 3 and r[7] == 1
    first = run.tab.raw()
    # fewer rows than components: the first ones, and nothing behind them
    run.stats(K - 2, rows=K)
    assert np.array_equal(run.tab.get()[:K - 2], want['rows'][:K - 2]) and run.tab.is_sentinel(slice(K - 2, K))
    run.stats(0, rows=K)                                             # n_comp == 0: nothing written, table may be NULL
    assert run.tab.untouched()
    a = run.mesh_args(True)
    _call('ofx_mesh_cc_stats', a[0], a[1], run.ints.ptr(0), a[2], a[3], *run.sizes, 0, None, run.ws.ptr, run.status.ptr)
    run.stats(K)
    assert np.array_equal(run.tab.raw(), first) and run.guards()


# ------------------------------------------------------------------------------------------------ select
def _tetra_at(origin, size):
    return (U.TETRA_V * np.asarray(size, np.float32) + np.asarray(origin, np.float32)).astype(np.float32)


def test_select_ties():
    f2 = np.concatenate([U.TETRA_F, U.TETRA_F + 4]).astype(np.int32)
    lo, hi = np.float32(0.1), np.float32(1.1)
    assert np.float32(hi - lo) == np.float32(1.0) and float(hi) - float(lo) > 1.0       # a tie in fp32 only
    a = _tetra_at((0, 0, 0), (1, 0.5, 0.5))                          # extent exactly 1 along x
    b = np.array([[lo, 3, 3], [hi, 3, 3], [lo, 3.5, 3], [lo, 3, 3.5]], np.float32)      # 1.1f - 0.1f along x
    c = _tetra_at((0, 0, 8), (0.25, 0.5, 1))                         # extent 1 along z
    small = _tetra_at((20, 20, 20), (0.5, 0.5, 0.5))
    big = _tetra_at((30, 30, 30), (0.5, 2, 0.5))
    meshes = [(np.concatenate([a, b]), f2),                          # fp32 tie: the lower label, a
              (np.concatenate([b, a]), f2),                          # ... whichever comes first
              (np.concatenate([c, a]), f2),                          # a tie on different axes
              (np.concatenate([small, big]), f2),                    # no tie: the later one wins
              (np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int32)),        # no faces
              (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)),        # nothing
              (np.concatenate([small, a, c]), np.concatenate([f2, U.TETRA_F + 8]).astype(np.int32))]
    run, want = check_twice(meshes, gaps=6)
    assert run.ints.get(3).tolist() == [0, 0, 0, 4, -1, -1, 4]
    keep = run.keep.get().reshape(3, len(meshes)).T
    assert keep[:, 2].tolist() == [2, 2, 2, 2, 0, 0, 3] and keep[:, 0].tolist() == [4, 4, 4, 4, 0, 0, 4]


# ------------------------------------------------------------------------------------------------ status
def _two_tetras():
    v, f = U.tiny_shape('tetra', np.random.default_rng(0))
    return [(v, f), U.tiny_shape('pair', np.random.default_rng(1))]


def test_status_on_entry_stops_table_stats_select_extract():
    run = CcRun(_two_tetras()).label()
    assert run.status.get().tolist() == [0, 0]
    label = run.ints.get(0)
    run.status.set([0, 1])
    run.table()
    run.stats(3)
    run.select()
    run.extract(np.array([[4, 4, 1], [4, 4, 2]]), gaps=1)
    torch.cuda.synchronize()
    assert np.array_equal(run.ints.get(0), label)
    for i in (1, 2, 3):
        assert bool((run.ints.view(i) == U.SENT[I32]).all())
    assert run.tab.untouched() and run.keep.untouched() and run.out_v.untouched() and run.out_f.untouched()
    assert run.status.get().tolist() == [0, 1] and run.guards()
    # and with the status cleared the same buffers fill
    run.status.set([0, 0])
    run.table().select()
    assert run.ints.get(2).tolist() == [0, 1, 3] and run.ints.get(3).tolist() == [0, 0]


@pytest.mark.parametrize('case', ['vert_off0', 'tri_off0', 'descending_vert', 'descending_tri', 'last_vert',
                                  'last_tri'])
def test_status_inconsistent_offsets(case):
    v, f, voff, toff = U.cat(_two_tetras())
    voff, toff = voff.copy(), toff.copy()
    if case == 'vert_off0':
        voff[0] = 1
    elif case == 'tri_off0':
        toff[0] = 1
    elif case == 'descending_vert':
        voff[1] = voff[2] + 1                                        # 0, 13, 12
    elif case == 'descending_tri':
        toff[1] = toff[2] + 1                                        # 0, 13, 12
    elif case == 'last_vert':
        voff[2] -= 1
    else:
        toff[2] -= 1
    run = CcRun(raw=(v, f, voff, toff)).label()
    st = run.status.get().tolist()                                   # bit 0 may come with it: the faces are judged
    assert st[0] == 0 and st[1] & 2 and st[1] < 4                    # against the table as it stands
    assert bool((run.ints.view(0) == U.SENT[I32]).all())             # no later pass touched the mesh: no label
    run.table()
    torch.cuda.synchronize()
    assert run.ints.untouched() and run.guards()


def test_status_index_equal_to_the_shapes_vertex_count():
    v, f, voff, toff = U.cat(_two_tetras())
    f = f.copy()
    f[2, 1] = 4                                                      # shape 0 has vertices 0 .. 3; 4 exists in the batch
    run = CcRun(raw=(v, f, voff, toff)).label()
    assert run.status.get().tolist() == [0, 1]
    run.table()
    torch.cuda.synchronize()
    assert run.ints.untouched() and run.guards()
    f[2, 1] = -1
    assert CcRun(raw=(v, f, voff, toff)).label().status.get().tolist() == [0, 1]
    f[2, 1] = 3
    assert CcRun(raw=(v, f, voff, toff)).label().status.get().tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    ws = lib().ofx_mesh_cc_ws_bytes
    assert ws(0, 5, 1) == 0 and ws(5, 0, 1) == 0 and ws(5, 5, 0) == 0 and ws(5, 5, -1) == 0
    assert ws(2 ** 31, 5, 1) == 0 and ws(5, 2 ** 31, 1) == 0 and ws(-1, 5, 1) == 0 and ws(5, 5, 1) > 0
    run = CcRun(_two_tetras())
    run.stats(0, rows=3)                                             # the table buffer; n_comp == 0 launches nothing
    run.out_v, run.out_f, new = Guarded(8, F32, cols=3), Guarded(8, I32, cols=3), up(np.zeros(4), I64)
    m, mv, S = run.mesh_args(), run.mesh_args(True), run.sizes
    lab, cov, coff, win = (run.ints.ptr(i) for i in range(4))
    w, st = run.ws.ptr, run.status.ptr
    calls = {
        'ofx_mesh_cc_label': ([*m, *S, lab, w, st], (0, 1, 2, 6, 7, 8)),
        'ofx_mesh_cc_table': ([m[0], lab, m[1], m[2], *S, cov, coff, w, st], (0, 1, 2, 3, 8, 9, 10)),
        'ofx_mesh_cc_stats': ([mv[0], mv[1], lab, mv[2], mv[3], *S, 3, run.tab.ptr, w, st], (0, 1, 2, 3, 4, 9, 10, 11)),
        'ofx_mesh_cc_select': ([mv[0], mv[1], lab, mv[2], mv[3], *S, win, run.keep.ptr, w, st],
                               (0, 1, 2, 3, 4, 8, 9, 10, 11)),
        'ofx_mesh_cc_extract': ([*mv, *S, new.data_ptr(), new.data_ptr(), run.out_v.ptr, run.out_f.ptr, w, st],
                                (0, 1, 2, 3, 7, 8, 9, 10, 11, 12)),
    }
    for name, (good, nulls) in calls.items():
        for i in nulls:
            a = list(good)
            a[i] = None
            _refused(name, *a)
        at = good.index(S[0])                                        # batch, V, F follow each other
        assert good[at:at + 3] == list(S)
        for j, bad in ((0, 0), (1, 0), (2, 0), (1, 2 ** 31), (2, 2 ** 31)):
            a = list(good)
            a[at + j] = bad
            _refused(name, *a)
    a = list(calls['ofx_mesh_cc_stats'][0])
    a[8] = -1                                                        # n_comp < 0
    _refused('ofx_mesh_cc_stats', *a)
    settled(run.ws, run.status, run.keep, run.tab, run.out_v, run.out_f)
    assert run.ints.untouched()
