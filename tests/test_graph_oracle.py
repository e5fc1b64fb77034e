"""tests/graph_oracle.py on the host: the geometric graph equals oracle/dual_octree.py on the deep trees, the trees have
the properties the GPU tests rely on (asserted as conditions), the vectorised table oracles equal the plain loops, and
every comparison the GPU tests make rejects a planted error.  No GPU, no octfusion_amd."""
import numpy as np
import pytest
import torch

import graph_oracle as G

torch.set_grad_enabled(False)

DEEP = ('deep_a', 'deep_b', 'deep_c')
FIVE = ('deep_a', 'deep_b', 'deep_b_mid', 'deep_c', 'full_face')


def _depths(name):
    oc, _ = G.tree(name)
    return range(oc.full_depth, oc.depth + 1)


def _n_rows(name, d):
    return int(G.tree(name)[1].graph[d]['node_type'].shape[0])


@pytest.mark.parametrize('name', FIVE + ('deep_b_last',))
def test_geometric_graph_equals_the_oracle(name):
    oc, o_doc = G.tree(name)
    assert oc.depth == oc.full_depth + 4
    ran = 0
    for d in _depths(name):
        if _n_rows(name, d) > G.GEOMETRIC_MAX:
            continue
        gp, gc = G.geometric_graph(oc, d)
        op, oc_ = G.csr_of_oracle(o_doc, d)
        assert np.array_equal(gp, op) and np.array_equal(gc, oc_), (name, d)
        # rows and attributes: the oracle's own node_type / keyd / mask / batch id
        A = G.node_attributes(oc, d)
        g = o_doc.graph[d]
        assert np.array_equal(A['node_type'], g['node_type'].numpy())
        assert np.array_equal(A['keyd'], g['keyd'].numpy())
        assert np.array_equal(A['node_mask'], g['node_mask'].long().numpy())
        assert A['node_mask'].shape[0] == int(o_doc.ncum[d] + o_doc.nnum[d] - o_doc.ncum[oc.full_depth])
        assert np.array_equal(A['batch_id'], o_doc.batch_id(d).numpy())
        ran += 1
    assert ran >= 3, ran


def test_the_empty_element_moves():
    for name, empty in (('deep_b', 0), ('deep_b_mid', 1), ('deep_b_last', 2)):
        oc, o_doc = G.tree(name)
        bid = o_doc.batch_id(oc.depth)
        per = torch.bincount(bid, minlength=3)
        assert int(per[empty]) == 8 ** oc.full_depth and all(int(per[b]) > 1000 for b in range(3) if b != empty)


@pytest.mark.parametrize('name', ('deep_a', 'deep_b', 'deep_b_mid', 'deep_b_last'))
def test_deep_trees_have_large_segments(name):
    """The depth-6 deep trees: a multi-neighbour segment of at least 64 rows (four times what any shallower test tree
    holds).  `deep_c` is there for its depth (7, one element); its recipe gives 61, pinned below."""
    oc, _ = G.tree(name)
    seg_ptr, col, N = G.tree_csr(name, oc.depth)
    assert int(G.seg_sizes(seg_ptr).max()) >= 64


def test_deep_c_is_seven_deep():
    oc, o_doc = G.tree('deep_c')
    assert (oc.depth, oc.full_depth, oc.batch_size) == (7, 3, 1)
    seg_ptr, col, N = G.tree_csr('deep_c', 7)
    assert N == 15723 and int(G.seg_sizes(seg_ptr).max()) == 61


def test_full_face_has_nine_segments_of_256():
    oc, _ = G.tree('full_face')
    assert [int(v) for v in oc.nnum] == [2, 16, 128, 16, 128, 1024, 8192]
    for d, want in ((6, 256), (5, 64), (4, 16), (3, 4)):
        seg_ptr, col, N = G.tree_csr('full_face', d)
        n = G.seg_sizes(seg_ptr)
        assert int(n.max()) == want and int((n == want).sum()) == 9, (d, int(n.max()), int((n == want).sum()))
    # ... all of one node type: what a byte-wide counter per type cannot hold
    seg_ptr, col, N = G.tree_csr('full_face', 6)
    ntype = G.node_attributes(oc, 6)['node_type']
    for s in np.nonzero(G.seg_sizes(seg_ptr) == 256)[0]:
        assert set(ntype[col[seg_ptr[s]:seg_ptr[s + 1]]].tolist()) == {4}


def test_leaf_prefix_and_spread_of_the_sources():
    odd_prefix = spread = 0
    for name in FIVE:
        oc, o_doc = G.tree(name)
        for d in _depths(name):
            N = _n_rows(name, d)
            odd_prefix += (N - int(oc.nnum[d])) % 8 != 0
        seg_ptr, col, N = G.tree_csr(name, oc.depth)
        for s in np.nonzero(G.seg_sizes(seg_ptr) > 1)[0]:
            c = col[seg_ptr[s]:seg_ptr[s + 1]]
            spread += len(set((c // 64).tolist())) > 1 and len(set((c // 8).tolist())) > 1
    assert odd_prefix >= 1, 'no graph depth with a leaf prefix that is not a multiple of 8'
    assert spread >= 1, 'no segment whose sources span several 64-row blocks and several octets'


# ---------------------------------------------------------------------------------------------- table oracles
_hand_csr = G.hand_csr


def test_fast_forms_equal_the_loops():
    for seed, n_nodes in ((0, 37), (1, 1), (2, 5)):
        seg_ptr, col = _hand_csr(seed, n_nodes)
        ntype = np.random.default_rng(seed).integers(0, 8, size=n_nodes)
        assert np.array_equal(G.primary(seg_ptr, col), G.primary_fast(seg_ptr, col))
        a, b = G.primary_ext(seg_ptr, col, n_nodes), G.primary_ext_fast(seg_ptr, col, n_nodes)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(G.multi_flag(seg_ptr), (G.seg_sizes(seg_ptr) > 1).astype(np.int64))
        for nt in (1, 5, 8):
            a, b = G.type_frac(seg_ptr, col, ntype, nt), G.type_frac_fast(seg_ptr, col, ntype, nt)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert all(np.array_equal(x, y) for x, y in zip(G.expand(seg_ptr, col), G.expand_fast(seg_ptr, col)))
        a, b = G.reverse(seg_ptr, col, n_nodes), G.reverse_fast(seg_ptr, col, n_nodes)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[2].dtype == np.float32
        w = G.hand_weights(seed, col.shape[0])
        assert np.array_equal(G.primary_w(seg_ptr, col, w), G.primary_w_fast(seg_ptr, col, w))
        assert np.array_equal(G.multi_flag_w(seg_ptr, w), G.multi_flag_w_fast(seg_ptr, w))
        a, b = G.primary_ext_w(seg_ptr, col, w, n_nodes + 3), G.primary_ext_w_fast(seg_ptr, col, w, n_nodes + 3)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert int((G.multi_flag_w(seg_ptr, w) != G.multi_flag(seg_ptr)).sum()) > 0 or n_nodes == 1
    for fn in (G.primary_fast, lambda p, c: G.primary_ext_fast(p, c, 0)[0]):          # no segment at all
        assert fn(*G.hand_csr(0, 0)).shape == (0,)
    # unweighted == weighted with all weights 1
    seg_ptr, col = _hand_csr(3, 9)
    ones = np.ones(col.shape[0], dtype=np.float32)
    assert np.array_equal(G.primary(seg_ptr, col), G.primary_w(seg_ptr, col, ones))
    assert np.array_equal(G.multi_flag(seg_ptr), G.multi_flag_w(seg_ptr, ones))
    a, b = G.primary_ext(seg_ptr, col, 9), G.primary_ext_w(seg_ptr, col, ones, 9)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_reverse_of_a_tree_transposes_it():
    """on a dual-octree graph: the reverse of the reverse structure names the forward edges again"""
    seg_ptr, col, N = G.tree_csr('deep_a', 4)
    rev_ptr, rev_row, rev_w = G.reverse_fast(seg_ptr, col, N)
    assert int(rev_ptr[-1]) == int(seg_ptr[-1])
    back = G.reverse_fast(rev_ptr, rev_row, N)
    assert np.array_equal(back[0], seg_ptr) and np.array_equal(back[1], G.sort_segments(seg_ptr, col))
    n = G.seg_sizes(seg_ptr)
    assert float(rev_w.min()) == float(np.float32(1.0) / np.float32(n.max()))


def test_planted_swapped_column_is_rejected():
    seg_ptr, col, N = G.tree_csr('deep_a', 4)
    assert G.csr_equal(seg_ptr, col, seg_ptr, col)
    shuffled = col.copy()                                          # another order INSIDE a segment is the same graph
    s = int(np.argmax(G.seg_sizes(seg_ptr)))
    a, e = int(seg_ptr[s]), int(seg_ptr[s + 1])
    shuffled[a:e] = shuffled[a:e][::-1]
    assert not np.array_equal(shuffled, col) and G.csr_equal(seg_ptr, shuffled, seg_ptr, col)
    bad = col.copy()                                               # the same column moved to the neighbouring segment
    assert col[a - 1] != col[a]
    bad[a - 1], bad[a] = col[a], col[a - 1]
    assert not G.csr_equal(seg_ptr, bad, seg_ptr, col)
    bad_ptr = seg_ptr.copy()
    bad_ptr[s] += 1
    assert not G.csr_equal(bad_ptr, col, seg_ptr, col)


def test_planted_rank_error_is_rejected():
    """primary_ext / leafrank on inputs small enough to number by hand; an implementation that ranks with an inclusive
    scan (the planted error) is told apart by the comparison the GPU tests make"""
    seg_ptr = np.array([0, 2, 2, 3, 6, 8, 8, 9], dtype=np.int64)          # sizes 2 0 1 3 2 0 1
    col = np.array([3, 1, 2, 0, 1, 2, 3, 0, 1], dtype=np.int64)
    want_ext, want_multi = [5, 4, 2, 6, 7, 4, 1], [0, 3, 4]               # n_src = 4: zero row 4, aux rows from 5
    for fn in (G.primary_ext, G.primary_ext_fast):
        ext, multi = fn(seg_ptr, col, 4)
        assert ext.tolist() == want_ext and multi.tolist() == want_multi, fn.__name__
    assert G.primary(seg_ptr, col).tolist() == [-2, -1, 2, -2, -2, -1, 1]

    def inclusive(seg_ptr, col, n_src):                                    # the planted error
        n = G.seg_sizes(seg_ptr)
        rank = np.cumsum(n > 1)
        return np.where(n == 0, n_src, np.where(n == 1, G.primary_fast(seg_ptr, col), n_src + 1 + rank))
    for sp, cl, n_src in ((seg_ptr, col, 4),) + tuple(G.hand_csr(s, n) + (n,) for s, n in ((4, 11), (5, 37))):
        bad, good = inclusive(sp, cl, n_src), G.primary_ext(sp, cl, n_src)[0]
        multi = G.seg_sizes(sp) > 1
        assert not np.array_equal(bad, good) and np.array_equal(bad[multi], good[multi] + 1)
    # leafrank by hand: children -1 = leaf
    class Tiny:
        depth = 1
        children = [torch.tensor([0]), torch.tensor([-1, 0, -1, -1, 1, -1, 2, -1])]
    assert G.leafrank(Tiny).tolist() == [0] + [0, 1, 1, 2, 3, 3, 4, 4]
    oc, _ = G.tree('deep_a')
    want = np.concatenate([np.cumsum(c.numpy() < 0) - (c.numpy() < 0) for c in oc.children])
    assert np.array_equal(G.leafrank(oc), want)
    inclusive_rank = np.concatenate([np.cumsum(c.numpy() < 0) for c in oc.children])    # the planted error
    assert not np.array_equal(inclusive_rank, G.leafrank(oc))


def test_planted_weight_treated_as_simple_is_rejected():
    seg_ptr = np.array([0, 1, 2, 2, 4], dtype=np.int64)
    col = np.array([5, 6, 7, 8], dtype=np.int64)
    w = np.array([1.0, 0.25, 1.0, 1.0], dtype=np.float32)
    assert G.primary_w(seg_ptr, col, w).tolist() == [5, -2, -1, -2]
    assert G.multi_flag_w(seg_ptr, w).tolist() == [0, 1, 0, 1]
    ext, multi = G.primary_ext_w(seg_ptr, col, w, 9)
    assert ext.tolist() == [5, 10, 9, 11] and multi.tolist() == [1, 3]
    # the unweighted tables are what an implementation that ignores the weight would give: they differ
    assert G.primary(seg_ptr, col).tolist() != G.primary_w(seg_ptr, col, w).tolist()
    assert G.multi_flag(seg_ptr).tolist() != G.multi_flag_w(seg_ptr, w).tolist()
    assert G.primary_ext(seg_ptr, col, 9)[0].tolist() != ext.tolist()
    # a weight that merely rounds to 1 in a narrower format is not 1
    w2 = np.array([np.nextafter(np.float32(1), np.float32(0)), 0.25, 1.0, 1.0], dtype=np.float32)
    assert G.primary_w(seg_ptr, col, w2).tolist()[0] == -2


def test_planted_reverse_order_is_rejected():
    """the reverse CSR of a graph small enough to transpose by hand, rows 3, 0 and 2 naming one column in one
    direction; an implementation that keeps a reverse segment in arrival order (the planted error: here descending
    rows) has the right rows and weights and is still rejected"""
    n = 4
    sizes = np.zeros(n * 7, dtype=np.int64)
    sizes[[0 * 7 + 2, 2 * 7 + 2, 3 * 7 + 2, 1 * 7 + 5]] = [1, 4, 2, 1]
    seg_ptr = G.exclusive_scan(sizes)
    # in segment order: (0, dir 2) -> 1 | (1, dir 5) -> 2 | (2, dir 2) -> 1 0 3 2 | (3, dir 2) -> 1 0
    col = np.array([1, 2, 1, 0, 3, 2, 1, 0], dtype=np.int64)
    want = {(1, 2): ([0, 2, 3], [1.0, 0.25, 0.5]), (0, 2): ([2, 3], [0.25, 0.5]), (3, 2): ([2], [0.25]),
            (2, 2): ([2], [0.25]), (2, 5): ([1], [1.0])}
    for fn in (G.reverse, G.reverse_fast):
        rev_ptr, rev_row, rev_w = fn(seg_ptr, col, n)
        assert rev_w.dtype == np.float32 and int(rev_ptr[-1]) == 8
        for c in range(n):
            for d in range(7):
                a, e = int(rev_ptr[c * 7 + d]), int(rev_ptr[c * 7 + d + 1])
                rows, ws = want.get((c, d), ([], []))
                assert rev_row[a:e].tolist() == rows and rev_w[a:e].tolist() == ws, (fn.__name__, c, d)

    def arrival_order(seg_ptr, col, n_nodes):                              # the planted error: last writer first
        rev_ptr, rev_row, rev_w = G.reverse_fast(seg_ptr, col, n_nodes)
        row, w = rev_row.copy(), rev_w.copy()
        for s in range(n_nodes * 7):
            a, e = int(rev_ptr[s]), int(rev_ptr[s + 1])
            row[a:e], w[a:e] = rev_row[a:e][::-1], rev_w[a:e][::-1]
        return rev_ptr, row, w
    good, bad = G.reverse(seg_ptr, col, n), arrival_order(seg_ptr, col, n)
    assert np.array_equal(good[0], bad[0]) and not np.array_equal(good[1], bad[1]) and not np.array_equal(good[2], bad[2])
    sp, cl, N = G.tree_csr('deep_a', 4)
    good, bad = G.reverse_fast(sp, cl, N), arrival_order(sp, cl, N)
    assert not np.array_equal(good[1], bad[1]) and np.array_equal(np.sort(good[1]), np.sort(bad[1]))


def test_type_frac_bound_accepts_two_roundings():
    """float(c) * (1.f / float(n)) against c / n: within 1.01 * 2^-23 * c / n, equal when n is a power of two"""
    worst = 0.0
    for n in list(range(1, 300)) + [1000, 1 << 10, 4096]:
        c = np.arange(0, n + 1, dtype=np.int64)
        got = (c.astype(np.float32) * (np.float32(1.0) / np.float32(n))).astype(np.float64)
        ref = c.astype(np.float64) / float(n)
        assert np.all(np.abs(got - ref) <= 1.01 * 2.0 ** -23 * ref), n
        if n & (n - 1) == 0:
            assert np.array_equal(got, ref), n
        worst = max(worst, float((np.abs(got - ref)[1:] / ref[1:]).max()) * 2.0 ** 23)
    assert 0.5 < worst <= 1.01, worst                              # the bound is neither loose nor missed
