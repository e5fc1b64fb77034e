"""The dual-octree graph build and every table derived from it (csrc/ofx_graph.hip), one entry point at a time through
the C ABI, against tests/graph_oracle.py -- bit for bit.

  * ofx_tree_leafrank, ofx_graph_nodes, ofx_graph_count -> ops.scan_i32 -> ofx_graph_fill on every graph depth of trees
    four levels deeper than their full layer (multi-neighbour segments of 61 .. 256 rows; an empty batch element first,
    in the middle and last; one element at depth 7), on d == full_depth and on a tree that IS its full layer.  The
    `_lib.OfxTree` is filled from the ORACLE octree's arrays: nothing of octree.py / dual_octree.py takes part.  Columns
    are compared as the sorted contents of each (row, dir) segment (the order inside one is unspecified in the reference,
    dual_octree.py:332-341); two builds give the same bits.
  * the derived-table entry points on hand-made CSRs that are no trees: segments of 0, 1, 2, 255, 256 and 1000 entries;
    0, 1, 37 and 299 600 nodes (2 097 200 segments: one more than the 8192 x 256 threads ofx_grid launches, so the
    grid-stride loops take their second pass); ofx_seg_* with a segment count that is no multiple of 7 and n_src != nseg.
  * refusals: every NULL a table builder must reject, d outside [full_depth, depth], a tree without leaf ranks.

Outputs sit inside sentinel-filled buffers whose guard bands must come back untouched.  type_frac is the one comparison
with a bound: the kernel computes float(c) * (1.f / float(n)), two roundings against c / n, so |got - c / n| <= 1.01 *
2^-23 * c / n elementwise, and equality where n is a power of two (tests/test_graph_oracle.py shows the bound holds for
that arithmetic and is not loose).  rev_w must equal float32(1) / float32(size): both are one correctly rounded division.
"""
import ctypes

import numpy as np
import pytest
import torch

import graph_oracle as G
from test_gpu_fullwidth import dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

GRID_CAP = 8192 * 256
PAD = 64
SENT = {torch.int32: -1234567, torch.int64: -123456789012, torch.uint8: 0xA5, torch.float32: -12345.678}


class Guarded:
    """`n` elements between two sentinel bands of PAD elements; `.ptr` points at the first of the n."""

    def __init__(self, n, dtype):
        self.n, self.dtype = int(n), dtype
        self.buf = torch.full((self.n + 2 * PAD,), SENT[dtype], dtype=dtype, device=dev())
        self.view = self.buf[PAD:PAD + self.n]
        self.ptr = self.view.data_ptr() if self.n else self.buf.data_ptr() + PAD * self.buf.element_size()

    def bands_intact(self):
        want = torch.full((PAD,), SENT[self.dtype], dtype=self.dtype, device=dev())
        return torch.equal(self.buf[:PAD], want) and torch.equal(self.buf[PAD + self.n:], want)

    def untouched(self):
        return torch.equal(self.buf, torch.full_like(self.buf, SENT[self.dtype]))

    def get(self):
        assert self.bands_intact(), 'wrote outside its extent'
        a = self.view.cpu().numpy()
        return a.astype(np.int64) if self.dtype != torch.float32 else a


def _up(a, dtype):
    """host array -> device tensor of at least one element (an empty tensor has a NULL data pointer)"""
    t = torch.as_tensor(np.ascontiguousarray(a)).to(dtype)
    if t.numel() == 0:
        return torch.zeros(1, dtype=dtype, device=dev())[:0], torch.zeros(1, dtype=dtype, device=dev())
    t = t.to(dev())
    return t, t


def _p(pair):
    """device pointer of _up's result (the backing tensor when the logical one is empty)"""
    return pair[1].data_ptr()


# =============================================================================================== the tree build
class DevTree:
    """The oracle octree's arrays on the device behind an `_lib.OfxTree`; leaf ranks by ofx_tree_leafrank."""

    def __init__(self, oc, leafrank=True):
        from octfusion_amd import _lib
        from octfusion_amd._lib import call, stream
        self.oc = oc
        depth = oc.depth
        self.child = torch.cat([oc.children[t] for t in range(depth + 1)]).to(torch.int32).to(dev())
        self.key = torch.cat([oc.keys[t] for t in range(depth + 1)]).to(torch.int64).to(dev())
        self.nnum = [int(oc.nnum[t]) for t in range(depth + 1)]
        self.nne = [int(oc.nnum_nempty[t]) for t in range(depth + 1)]
        self.ncum = [0] + np.cumsum(self.nnum).tolist()
        self._nnum_c = (ctypes.c_int64 * (depth + 1))(*self.nnum)
        self._nne_c = (ctypes.c_int64 * (depth + 1))(*self.nne)
        total = self.ncum[-1]
        assert self.child.numel() == total == self.key.numel()
        self.rank = Guarded(total, torch.int32)
        ws = torch.empty(_lib.lib().ofx_tree_leafrank_ws_bytes(max(self.nnum)), dtype=torch.uint8, device=dev())
        call('ofx_tree_leafrank', self.child.data_ptr(), ctypes.addressof(self._nnum_c), depth, self.rank.ptr,
             ws.data_ptr(), stream())
        self.tree = self.struct(leafrank=leafrank)

    def struct(self, leafrank=True, depth=None, full_depth=None):
        from octfusion_amd import _lib
        oc = self.oc
        return _lib.OfxTree(oc.depth if depth is None else depth, oc.full_depth if full_depth is None else full_depth,
                            oc.batch_size, self.child.data_ptr(), self.key.data_ptr(), self.rank.ptr if leafrank else None,
                            ctypes.addressof(self._nnum_c), ctypes.addressof(self._nne_c))

    def rows(self, d):
        fd = self.oc.full_depth
        return sum(self.nnum[t] - self.nne[t] for t in range(fd, d)) + self.nnum[d]

    def mask_len(self, d):
        return self.ncum[d] + self.nnum[d] - self.ncum[self.oc.full_depth]


_DEV_TREES = {}


def _dev_tree(name):
    if name not in _DEV_TREES:
        _DEV_TREES[name] = DevTree(_oracle_tree(name)[0])
    return _DEV_TREES[name]


def _oracle_tree(name):
    if name == 'full_layer':                      # a tree whose depth IS its full depth: two dense 4^3 grids
        return _full_layer()
    return G.tree(name)


_FULL = []


def _full_layer():
    if not _FULL:
        from oracle import dual_octree as OD, sampler as OS
        oc = OS.create_full_octree(2, 2, 2)
        o_doc = OD.OracleDualOctree(oc)
        o_doc.post_processing_for_docnn()
        _FULL.append((oc, o_doc))
    return _FULL[0]


def _want_csr(name, d):
    if name == 'full_layer':
        oc, o_doc = _full_layer()
        seg_ptr, col = G.geometric_graph(oc, d)
        op, ocol = G.csr_of_oracle(o_doc, d)
        assert np.array_equal(seg_ptr, op) and np.array_equal(col, ocol)
        return seg_ptr, col, 128
    return G.tree_csr(name, d)


def _build(T, d):
    """count -> scan -> fill through the C ABI; (seg_cnt, seg_ptr, col) as int64 host arrays + the device col"""
    from octfusion_amd import ops
    from octfusion_amd._lib import call, stream
    N = T.rows(d)
    cnt = Guarded(N * 7, torch.int32)
    call('ofx_graph_count', ctypes.byref(T.tree), d, cnt.ptr, stream())
    seg_ptr = ops.scan_i32(cnt.view)
    E = int(seg_ptr[-1])
    col = Guarded(E, torch.int32)
    call('ofx_graph_fill', ctypes.byref(T.tree), d, seg_ptr.data_ptr(), col.ptr, stream())
    return cnt.get(), seg_ptr.cpu().numpy().astype(np.int64), col.get(), col


TREE_DEPTHS = [(name, fd + k) for name, fd in (('deep_a', 2), ('deep_b', 2), ('deep_b_mid', 2), ('deep_b_last', 2),
                                               ('deep_c', 3), ('full_face', 2)) for k in range(5)] + [('full_layer', 2)]


def test_leafrank():
    for name in ('deep_a', 'deep_b', 'deep_c', 'full_face', 'full_layer'):
        T = _dev_tree(name)
        assert np.array_equal(T.rank.get(), G.leafrank(T.oc)), name


@pytest.mark.parametrize('name,d', TREE_DEPTHS, ids=lambda v: str(v))
def test_graph_build(name, d):
    from octfusion_amd._lib import call, stream
    T = _dev_tree(name)
    oc = T.oc
    assert oc.full_depth <= d <= oc.depth
    want_ptr, want_col, N = _want_csr(name, d)
    assert T.rows(d) == N
    cnt, seg_ptr, col, col_dev = _build(T, d)
    assert np.array_equal(cnt, G.seg_sizes(want_ptr)), 'segment sizes'
    assert np.array_equal(seg_ptr, want_ptr)
    assert np.array_equal(G.sort_segments(seg_ptr, col), want_col), 'columns of a segment'
    assert G.csr_equal(seg_ptr, col, want_ptr, want_col)
    _, _, _, col2 = _build(T, d)
    assert torch.equal(col_dev.buf, col2.buf), 'two builds differ'
    # node attributes: all four outputs, then each output NULL in turn
    A = G.node_attributes(oc, d)
    specs = [('batch_id', torch.int32, N), ('node_type', torch.uint8, N), ('keyd', torch.int64, N),
             ('node_mask', torch.uint8, T.mask_len(d))]
    assert A['node_mask'].shape[0] == T.mask_len(d)
    for skip in (None, 0, 1, 2, 3):
        outs = [Guarded(n, dt) for _, dt, n in specs]
        call('ofx_graph_nodes', ctypes.byref(T.tree), d, *[None if i == skip else o.ptr for i, o in enumerate(outs)],
             stream())
        for i, ((what, _, _), o) in enumerate(zip(specs, outs)):
            if i == skip:
                assert o.untouched(), what
            else:
                assert np.array_equal(o.get(), A[what]), (what, skip)


def test_graph_build_refusals():
    """d below the full layer, d beyond the tree, a tree without leaf ranks: OFX_EINVAL, nothing written"""
    from octfusion_amd import _lib
    from octfusion_amd._lib import call, stream
    T = _dev_tree('deep_a')
    fd, depth = T.oc.full_depth, T.oc.depth
    N = T.rows(depth)
    want_ptr, _, _ = G.tree_csr('deep_a', depth)
    seg_ptr = torch.as_tensor(want_ptr).to(torch.int32).to(dev())
    cnt, col = Guarded(N * 7, torch.int32), Guarded(int(want_ptr[-1]), torch.int32)
    outs = [Guarded(N, torch.int32), Guarded(N, torch.uint8), Guarded(N, torch.int64), Guarded(T.mask_len(depth), torch.uint8)]
    no_rank = T.struct(leafrank=False)
    for tree, d in ((T.tree, fd - 1), (T.tree, depth + 1), (T.tree, -1), (no_rank, depth), (no_rank, fd)):
        for go in (lambda: call('ofx_graph_count', ctypes.byref(tree), d, cnt.ptr, stream()),
                   lambda: call('ofx_graph_fill', ctypes.byref(tree), d, seg_ptr.data_ptr(), col.ptr, stream()),
                   lambda: call('ofx_graph_nodes', ctypes.byref(tree), d, *[o.ptr for o in outs], stream())):
            with pytest.raises(_lib.OfxError, match='invalid argument'):
                go()
    for bad in (lambda: call('ofx_graph_count', ctypes.byref(T.tree), depth, None, stream()),
                lambda: call('ofx_graph_fill', ctypes.byref(T.tree), depth, None, col.ptr, stream()),
                lambda: call('ofx_graph_fill', ctypes.byref(T.tree), depth, seg_ptr.data_ptr(), None, stream()),
                lambda: call('ofx_graph_count', None, depth, cnt.ptr, stream())):
        with pytest.raises(_lib.OfxError, match='invalid argument'):
            bad()
    torch.cuda.synchronize()
    assert all(o.untouched() for o in [cnt, col] + outs)


# =============================================================================================== derived tables
def _check_tables(seg_ptr, col, n_nodes, tag, type_cases=((1, 7), (1, 64), (5, 35), (5, 64), (8, 56), (8, 64))):
    """every node-keyed entry point on one CSR (int64 host arrays, columns in [0, n_nodes))"""
    from octfusion_amd import ops
    from octfusion_amd._lib import call, stream
    nseg = n_nodes * 7
    E = int(seg_ptr[-1])
    assert seg_ptr.shape[0] == nseg + 1 and col.shape[0] == E and (E == 0 or (0 <= col.min() and col.max() < n_nodes))
    sp, cl = _up(seg_ptr, torch.int32), _up(col, torch.int32)
    n = G.seg_sizes(seg_ptr)

    nbr = Guarded(nseg, torch.int32)
    call('ofx_graph_primary', _p(sp), _p(cl), n_nodes, nbr.ptr, stream())
    assert np.array_equal(nbr.get(), G.primary_fast(seg_ptr, col)), (tag, 'primary')

    flag = Guarded(nseg, torch.int32)
    call('ofx_graph_multi_flag', _p(sp), n_nodes, flag.ptr, stream())
    assert np.array_equal(flag.get(), (n > 1).astype(np.int64)), (tag, 'multi_flag')

    want_ext, want_multi = G.primary_ext_fast(seg_ptr, col, n_nodes)
    rank = ops.scan_i32(flag.view) if nseg else torch.zeros(1, dtype=torch.int32, device=dev())
    assert int(rank[-1]) == want_multi.shape[0]
    ext, multi = Guarded(nseg, torch.int32), Guarded(want_multi.shape[0], torch.int32)
    call('ofx_graph_primary_ext', _p(sp), _p(cl), n_nodes, rank.data_ptr(), ext.ptr, multi.ptr, stream())
    assert np.array_equal(ext.get(), want_ext), (tag, 'primary_ext')
    assert np.array_equal(multi.get(), want_multi), (tag, 'multi_seg')

    # expand: all three outputs, then each output NULL in turn
    want = G.expand_fast(seg_ptr, col)
    for skip in (None, 0, 1, 2):
        outs = [Guarded(E, torch.int64) for _ in range(3)]
        call('ofx_graph_expand', _p(sp), n_nodes, _p(cl), *[None if i == skip else o.ptr for i, o in enumerate(outs)],
             stream())
        for i, o in enumerate(outs):
            if i == skip:
                assert o.untouched(), (tag, 'expand', i)
            else:
                assert np.array_equal(o.get(), want[i]), (tag, 'expand', i, skip)

    # type_frac
    ntype = np.random.default_rng(n_nodes).integers(0, 8, size=n_nodes)
    nty = _up(ntype, torch.uint8)
    for nt, ld in type_cases:
        frac, cnt, n1 = G.type_frac_fast(seg_ptr, col, ntype, nt)
        tf = Guarded(n_nodes * ld, torch.float32)
        call('ofx_graph_type_frac', _p(sp), _p(cl), _p(nty), n_nodes, nt, tf.ptr, ld, stream())
        got = tf.get().reshape(n_nodes, ld).astype(np.float64)
        assert np.all(got[:, 7 * nt:] == 0.0), (tag, 'pad columns', nt, ld)
        got = got[:, :7 * nt].reshape(nseg, nt)
        err = np.abs(got - frac)
        assert np.all(err <= 1.01 * 2.0 ** -23 * frac), (tag, 'type_frac', nt, ld, float(err.max()))
        pow2 = (n1 & (n1 - 1)) == 0
        assert np.array_equal(got[pow2], frac[pow2]), (tag, 'type_frac at a power of two', nt, ld)

    # reverse CSR
    want_ptr, want_row, want_w = G.reverse_fast(seg_ptr, col, n_nodes)
    rcnt = Guarded(nseg, torch.int32)
    call('ofx_graph_reverse_count', _p(sp), _p(cl), n_nodes, rcnt.ptr, stream())
    if nseg:
        assert np.array_equal(rcnt.get(), G.seg_sizes(want_ptr)), (tag, 'reverse_count')
    else:
        assert rcnt.untouched()
    rev_ptr = _up(want_ptr, torch.int32)
    rev_row, rev_w = Guarded(E, torch.int32), Guarded(E, torch.float32)
    call('ofx_graph_reverse_fill', _p(sp), _p(cl), n_nodes, _p(rev_ptr), rcnt.ptr, rev_row.ptr, rev_w.ptr, stream())
    if nseg:
        assert np.array_equal(rev_row.get(), want_row), (tag, 'rev_row')
        got_w = rev_w.get()
        assert got_w.dtype == np.float32 and np.array_equal(got_w.view(np.int32), want_w.view(np.int32)), (tag, 'rev_w')
        assert np.array_equal(rcnt.get(), G.seg_sizes(want_ptr)), (tag, 'the cursor ends as the counts')
    else:
        assert rev_row.untouched() and rev_w.untouched()

    # the weighted builders on the reverse structure (weights 1 / size) and on drawn weights, node-keyed and segment-keyed
    _check_weighted(want_ptr, want_row, want_w, nseg, n_nodes, tag + ' reverse', node_keyed=True)
    _check_weighted(seg_ptr, col, G.hand_weights(n_nodes, E), nseg, n_nodes, tag + ' drawn', node_keyed=True)


def _check_weighted(seg_ptr, col, w, nseg, n_src, tag, node_keyed):
    from octfusion_amd import ops
    from octfusion_amd._lib import call, stream
    sp, cl, wd = _up(seg_ptr, torch.int32), _up(col, torch.int32), _up(w, torch.float32)
    forms = [('ofx_seg_', nseg, (n_src,))]
    if node_keyed:
        assert nseg % 7 == 0 and n_src == nseg // 7
        forms.append(('ofx_graph_', nseg // 7, ()))
    for prefix, count, src in forms:
        nbr = Guarded(nseg, torch.int32)
        call(prefix + 'primary_w', _p(sp), _p(cl), _p(wd), count, nbr.ptr, stream())
        assert np.array_equal(nbr.get(), G.primary_w_fast(seg_ptr, col, w)), (tag, prefix, 'primary_w')
        flag = Guarded(nseg, torch.int32)
        call(prefix + 'multi_flag_w', _p(sp), _p(wd), count, flag.ptr, stream())
        assert np.array_equal(flag.get(), G.multi_flag_w_fast(seg_ptr, w)), (tag, prefix, 'multi_flag_w')
        want_ext, want_multi = G.primary_ext_w_fast(seg_ptr, col, w, n_src)
        rank = ops.scan_i32(flag.view) if nseg else torch.zeros(1, dtype=torch.int32, device=dev())
        assert int(rank[-1]) == want_multi.shape[0]
        ext, multi = Guarded(nseg, torch.int32), Guarded(want_multi.shape[0], torch.int32)
        call(prefix + 'primary_ext_w', _p(sp), _p(cl), _p(wd), count, *src, rank.data_ptr(), ext.ptr, multi.ptr, stream())
        assert np.array_equal(ext.get(), want_ext), (tag, prefix, 'primary_ext_w')
        assert np.array_equal(multi.get(), want_multi), (tag, prefix, 'multi_seg')


@pytest.mark.parametrize('n_nodes', [0, 1, 37])
def test_tables_on_hand_made_csrs(n_nodes):
    seg_ptr, col = G.hand_csr(7 + n_nodes, n_nodes)
    if n_nodes:
        assert {0, 1, 2, 255, 256, 1000} <= set(G.seg_sizes(seg_ptr).tolist())
    _check_tables(seg_ptr, col, n_nodes, 'n=%d' % n_nodes)


def test_tables_past_the_grid_cap():
    """299 600 nodes = 2 097 200 segments: 48 more than the threads of the largest launch, so segments 2 097 152 ..
    are served by the second pass of the grid-stride loops -- and hold entries (asserted)"""
    n_nodes = 299600
    assert n_nodes * 7 == GRID_CAP + 48
    seg_ptr, col = G.hand_csr(5, n_nodes)
    assert int(seg_ptr[-1]) - int(seg_ptr[GRID_CAP]) > 8 and int(G.seg_sizes(seg_ptr)[GRID_CAP:].max()) == 2
    _check_tables(seg_ptr, col, n_nodes, 'n=299600', type_cases=((5, 35),))


def test_segment_keyed_tables():
    """ofx_seg_*: a segment count that is no multiple of 7, sources numbered independently of the segments"""
    for nseg, n_src in ((262, 50), (1, 9), (GRID_CAP + 5, 1000)):
        assert nseg % 7 != 0 and n_src != nseg
        seg_ptr, col = G.hand_csr(nseg, 0, nseg=nseg, n_src=n_src)
        w = G.hand_weights(nseg, col.shape[0])
        _check_weighted(seg_ptr, col, w, nseg, n_src, 'nseg=%d' % nseg, node_keyed=False)


def test_tables_of_a_deep_tree():
    """the same entry points on the graphs they are built for: full_face at depth 6 (nine segments of 256; every
    segment size a power of four) and deep_a at depth 5 (sizes up to 46 that are no powers of two)"""
    seg_ptr, col, N = G.tree_csr('full_face', 6)
    assert int(G.seg_sizes(seg_ptr).max()) == 256
    _check_tables(seg_ptr, col, N, 'full_face', type_cases=((5, 35), (8, 64)))
    seg_ptr, col, N = G.tree_csr('deep_a', 5)
    n = G.seg_sizes(seg_ptr)
    assert int(n.max()) == 46 and int(((n & (n - 1)) != 0).sum()) > 100
    _check_tables(seg_ptr, col, N, 'deep_a', type_cases=((5, 35),))


def test_table_refusals():
    """Every pointer of every table builder, NULL in turn: OFX_EINVAL from the host check, nothing launched, the
    outputs untouched.  (Each of these is rejected before any launch -- csrc/ofx_graph.hip; a NULL that reached a
    kernel would be dereferenced on the device.)  Then the same calls with every pointer in place go through."""
    from octfusion_amd import _lib, ops
    from octfusion_amd._lib import call, stream
    n_nodes = 5
    nseg = n_nodes * 7
    seg_ptr, col = G.hand_csr(11, n_nodes)
    E = int(seg_ptr[-1])
    w = G.hand_weights(11, E)
    sp, cl, wd = _up(seg_ptr, torch.int32), _up(col, torch.int32), _up(w, torch.float32)
    nty = _up(np.arange(n_nodes) % 5, torch.uint8)
    rank = ops.scan_i32(torch.as_tensor((G.seg_sizes(seg_ptr) > 1).astype(np.int32)).to(dev()))
    rank_w = ops.scan_i32(torch.as_tensor(G.multi_flag_w_fast(seg_ptr, w).astype(np.int32)).to(dev()))
    rev_ptr = _up(G.reverse_fast(seg_ptr, col, n_nodes)[0], torch.int32)
    o = dict(i1=Guarded(nseg, torch.int32), i2=Guarded(nseg, torch.int32), i3=Guarded(E, torch.int32),
             f1=Guarded(E, torch.float32), tf=Guarded(n_nodes * 35, torch.float32), l1=Guarded(E, torch.int64))
    S, Cc, W, R, RW, RP, NT = _p(sp), _p(cl), _p(wd), rank.data_ptr(), rank_w.data_ptr(), _p(rev_ptr), _p(nty)
    i1, i2, i3, f1, tf, l1 = (o[k].ptr for k in ('i1', 'i2', 'i3', 'f1', 'tf', 'l1'))
    # (entry point, arguments, positions of the pointers the host check must refuse when NULL)
    cases = [
        ('ofx_graph_primary', [S, Cc, n_nodes, i1], (0, 1, 3)),
        ('ofx_graph_multi_flag', [S, n_nodes, i1], (0, 2)),
        ('ofx_graph_primary_ext', [S, Cc, n_nodes, R, i1, i2], (0, 1, 3, 4, 5)),
        ('ofx_graph_type_frac', [S, Cc, NT, n_nodes, 5, tf, 35], (0, 1, 2, 5)),
        ('ofx_graph_expand', [S, n_nodes, Cc, None, l1, None], (0, 2)),
        ('ofx_graph_reverse_count', [S, Cc, n_nodes, i1], (0, 1, 3)),
        ('ofx_graph_reverse_fill', [S, Cc, n_nodes, RP, i1, i3, f1], (0, 1, 3, 4, 5, 6)),
        ('ofx_graph_primary_w', [S, Cc, W, n_nodes, i1], (0, 1, 2, 4)),
        ('ofx_graph_multi_flag_w', [S, W, n_nodes, i1], (0, 1, 3)),
        ('ofx_graph_primary_ext_w', [S, Cc, W, n_nodes, RW, i1, i2], (0, 1, 2, 4, 5, 6)),
        ('ofx_seg_primary_w', [S, Cc, W, nseg, i1], (0, 1, 2, 4)),
        ('ofx_seg_multi_flag_w', [S, W, nseg, i1], (0, 1, 3)),
        ('ofx_seg_primary_ext_w', [S, Cc, W, nseg, n_nodes, RW, i1, i2], (0, 1, 2, 5, 6, 7)),
    ]
    refused = 0
    for name, args, ptrs in cases:
        for k in ptrs:
            bad = list(args)
            bad[k] = None
            with pytest.raises(_lib.OfxError, match='invalid argument'):
                call(name, *bad, stream())
            refused += 1
        size_at = [i for i, a in enumerate(args) if a in (n_nodes, nseg) and i not in ptrs][0]
        bad = list(args)
        bad[size_at] = -1
        with pytest.raises(_lib.OfxError, match='invalid argument'):
            call(name, *bad, stream())
    for bad in ([S, Cc, NT, n_nodes, 0, tf, 35], [S, Cc, NT, n_nodes, 5, tf, 34]):           # nt < 1, ld < 7 nt
        with pytest.raises(_lib.OfxError, match='invalid argument'):
            call('ofx_graph_type_frac', *bad, stream())
    torch.cuda.synchronize()
    assert refused == sum(len(c[2]) for c in cases) == 51
    assert all(g.untouched() for g in o.values())
    for name, args, _ in cases:                                                     # valid: every one launches
        call(name, *args, stream())
    torch.cuda.synchronize()
    assert all(g.bands_intact() for g in o.values()) and not o['i1'].untouched()
