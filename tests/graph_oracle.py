"""Host restatements of the dual-octree graph and of every table derived from it (csrc/ofx_graph.hip), in plain
numpy / torch on the CPU.  TEST INFRASTRUCTURE: nothing here imports the product.

  * `geometric_graph(octree, d)`: the neighbour graph from geometry alone.  A row of graph depth d is a cube
    (lo = xyz << (d - t), size = 1 << (d - t) for a node of tree depth t); row j is a neighbour of row i through i's
    face `dir` when both lie in one batch element, j's cube starts where i's ends on that axis (or ends where i's
    starts) and the open intervals overlap on the two other axes.  O(N^2): it shares nothing with the kernel's walk down
    the child pointers, nor with the level-by-level refinement of oracle/dual_octree.py (reference
    models/networks/dualoctree_networks/dual_octree.py:124-239).  Use it for N <= GEOMETRIC_MAX rows.
  * the derived tables from a CSR (seg_ptr, col): primary / multi_flag / primary_ext (+ multi_seg) and their weighted
    forms, type_frac, expand, the reverse CSR; leafrank, node attributes and the node mask from the octree arrays.
    Loops over segments -- written for clarity, not speed; `n_nodes` in the millions goes through the vectorised
    `seg_sizes` forms, which tests/test_graph_oracle.py shows equal to the loops.
  * the deep ragged trees the GPU tests run on (`tree`), from tests/golden/common.py's recipes.

Direction codes (dual_octree.py:85-97, :247): 0:+z 1:-z 2:+y 3:-y 4:+x 5:-x 6:self.
"""
import functools

import numpy as np
import torch

GEOMETRIC_MAX = 9000
_AXIS_OF_DIR = (2, 2, 1, 1, 0, 0)            # dir -> index into (x, y, z)


# ------------------------------------------------------------------------------------------------ octree arrays
def _decode(key, depth):
    """Morton key -> (x, y, z, b): level bit i of x sits at key bit 3 i + 2, y at 3 i + 1, z at 3 i; batch id from bit 48."""
    key = np.asarray(key, dtype=np.int64)
    b = key >> 48
    k = key & ((1 << 48) - 1)
    x, y, z = np.zeros_like(k), np.zeros_like(k), np.zeros_like(k)
    for i in range(depth):
        x |= ((k >> (3 * i + 2)) & 1) << i
        y |= ((k >> (3 * i + 1)) & 1) << i
        z |= ((k >> (3 * i)) & 1) << i
    return x, y, z, b


def graph_rows(octree, d):
    """The rows of graph depth d, [leaves of depths fd..d-1 in tree order | all nodes of depth d]:
    dict of int64 arrays t (tree depth), j (index inside that depth), key, b, lo [N, 3], size."""
    fd = octree.full_depth
    assert fd <= d <= octree.depth
    ts, js, keys = [], [], []
    for t in range(fd, d + 1):
        key = octree.keys[t].numpy()
        child = octree.children[t].numpy()
        j = np.arange(key.shape[0], dtype=np.int64) if t == d else np.nonzero(child < 0)[0].astype(np.int64)
        ts.append(np.full(j.shape[0], t, dtype=np.int64))
        js.append(j)
        keys.append(key[j])
    t, j, key = np.concatenate(ts), np.concatenate(js), np.concatenate(keys)
    lo = np.zeros((t.shape[0], 3), dtype=np.int64)
    b = np.zeros(t.shape[0], dtype=np.int64)
    for tt in range(fd, d + 1):
        m = t == tt
        x, y, z, bb = _decode(key[m], tt)
        lo[m] = np.stack([x, y, z], 1) << (d - tt)
        b[m] = bb
    return dict(t=t, j=j, key=key, b=b, lo=lo, size=np.int64(1) << (d - t))


def geometric_graph(octree, d, chunk=1024):
    """(seg_ptr int64 [N * 7 + 1], col int64 [E]) of graph depth d, every segment in ascending column order."""
    R = graph_rows(octree, d)
    lo, b = R['lo'], R['b']
    hi = lo + R['size'][:, None]
    N = lo.shape[0]
    assert N <= GEOMETRIC_MAX, 'O(N^2): %d rows' % N
    rows, dirs, cols = [], [], []
    for i0 in range(0, N, chunk):
        i1 = min(i0 + chunk, N)
        same = b[i0:i1, None] == b[None, :]
        # open intervals overlap, per axis
        ov = [(lo[i0:i1, None, a] < hi[None, :, a]) & (lo[None, :, a] < hi[i0:i1, None, a]) for a in range(3)]
        for dr in range(6):
            a = _AXIS_OF_DIR[dr]
            o1, o2 = [k for k in range(3) if k != a]
            if dr % 2 == 0:                                       # + : j starts where i ends
                touch = lo[None, :, a] == hi[i0:i1, None, a]
            else:                                                 # - : j ends where i starts
                touch = hi[None, :, a] == lo[i0:i1, None, a]
            ii, jj = np.nonzero(same & touch & ov[o1] & ov[o2])   # row-major: ascending i, then ascending j
            rows.append(ii + i0)
            dirs.append(np.full(ii.shape[0], dr, dtype=np.int64))
            cols.append(jj)
    row, edir, col = np.concatenate(rows), np.concatenate(dirs), np.concatenate(cols)
    has_edge = np.zeros(N, dtype=bool)
    has_edge[row] = True
    self_rows = np.nonzero(has_edge)[0]
    row = np.concatenate([row, self_rows])
    edir = np.concatenate([edir, np.full(self_rows.shape[0], 6, dtype=np.int64)])
    col = np.concatenate([col, self_rows])
    return csr_from_edges(row, edir, col, N)


def csr_from_edges(row, edir, col, N):
    """COO (row, dir, col) -> (seg_ptr [N * 7 + 1], col), segments keyed row * 7 + dir, columns ascending inside."""
    row, edir, col = (np.asarray(v, dtype=np.int64) for v in (row, edir, col))
    order = np.lexsort((col, edir, row))
    seg = (row * 7 + edir)[order]
    seg_ptr = np.zeros(N * 7 + 1, dtype=np.int64)
    np.cumsum(np.bincount(seg, minlength=N * 7), out=seg_ptr[1:])
    return seg_ptr, col[order]


def csr_of_oracle(o_doc, d):
    """The same form from OracleDualOctree.graph[d] (after post_processing_for_docnn)."""
    g = o_doc.graph[d]
    N = int(g['node_type'].shape[0])
    return csr_from_edges(g['edge_idx'][0].numpy(), g['edge_dir'].numpy(), g['edge_idx'][1].numpy(), N)


def seg_sizes(seg_ptr):
    seg_ptr = np.asarray(seg_ptr, dtype=np.int64)
    return seg_ptr[1:] - seg_ptr[:-1]


def sort_segments(seg_ptr, col):
    """col with every segment sorted ascending (the order inside a segment is unspecified: dual_octree.py:332-341)."""
    seg_ptr, col = np.asarray(seg_ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    seg_of = np.repeat(np.arange(seg_ptr.shape[0] - 1, dtype=np.int64), seg_sizes(seg_ptr))
    return col[np.lexsort((col, seg_of))]


def csr_equal(ptr_a, col_a, ptr_b, col_b):
    """Same segment sizes and the same column multiset in every segment."""
    ptr_a, ptr_b = np.asarray(ptr_a, dtype=np.int64), np.asarray(ptr_b, dtype=np.int64)
    if ptr_a.shape != ptr_b.shape or not np.array_equal(ptr_a, ptr_b):
        return False
    if np.asarray(col_a).shape != np.asarray(col_b).shape:
        return False
    return bool(np.array_equal(sort_segments(ptr_a, col_a), sort_segments(ptr_b, col_b)))


# ------------------------------------------------------------------------------------------------ derived tables
def primary(seg_ptr, col):
    """nbr[s]: the single neighbour, -1 for an empty segment, -2 for several (ofx_graph_primary)."""
    nseg = len(seg_ptr) - 1
    out = np.empty(nseg, dtype=np.int64)
    for s in range(nseg):
        a, e = int(seg_ptr[s]), int(seg_ptr[s + 1])
        out[s] = -1 if e == a else (int(col[a]) if e - a == 1 else -2)
    return out


def multi_flag(seg_ptr):
    return np.array([1 if int(seg_ptr[s + 1]) - int(seg_ptr[s]) > 1 else 0 for s in range(len(seg_ptr) - 1)],
                    dtype=np.int64)


def exclusive_scan(v):
    """[n + 1]: out[i] = sum(v[:i]) (ofx_scan_i32)."""
    out = np.zeros(len(v) + 1, dtype=np.int64)
    np.cumsum(np.asarray(v, dtype=np.int64), out=out[1:])
    return out


def primary_ext(seg_ptr, col, n_src):
    """(nbr_ext, multi_seg): single neighbour -> its id; none -> n_src (the zero row); several -> n_src + 1 + v with v
    the rank of the segment among the multi-neighbour segments, multi_seg[v] = the segment (ofx_graph_primary_ext)."""
    nseg = len(seg_ptr) - 1
    out = np.empty(nseg, dtype=np.int64)
    multi = []
    for s in range(nseg):
        a, e = int(seg_ptr[s]), int(seg_ptr[s + 1])
        if e == a:
            out[s] = n_src
        elif e - a == 1:
            out[s] = int(col[a])
        else:
            out[s] = n_src + 1 + len(multi)
            multi.append(s)
    return out, np.array(multi, dtype=np.int64)


def _simple_w(seg_ptr, w, s):
    """a weighted segment is used as is only when it holds exactly one edge of weight exactly 1"""
    a, e = int(seg_ptr[s]), int(seg_ptr[s + 1])
    return e - a == 1 and float(w[a]) == 1.0


def primary_w(seg_ptr, col, w):
    nseg = len(seg_ptr) - 1
    out = np.empty(nseg, dtype=np.int64)
    for s in range(nseg):
        a, e = int(seg_ptr[s]), int(seg_ptr[s + 1])
        out[s] = -1 if e == a else (int(col[a]) if _simple_w(seg_ptr, w, s) else -2)
    return out


def multi_flag_w(seg_ptr, w):
    nseg = len(seg_ptr) - 1
    return np.array([0 if (int(seg_ptr[s + 1]) == int(seg_ptr[s]) or _simple_w(seg_ptr, w, s)) else 1
                     for s in range(nseg)], dtype=np.int64)


def primary_ext_w(seg_ptr, col, w, n_src):
    nseg = len(seg_ptr) - 1
    out = np.empty(nseg, dtype=np.int64)
    multi = []
    for s in range(nseg):
        a, e = int(seg_ptr[s]), int(seg_ptr[s + 1])
        if e == a:
            out[s] = n_src
        elif _simple_w(seg_ptr, w, s):
            out[s] = int(col[a])
        else:
            out[s] = n_src + 1 + len(multi)
            multi.append(s)
    return out, np.array(multi, dtype=np.int64)


def type_frac(seg_ptr, col, node_type, nt):
    """(frac float64 [nseg, nt] = c / n exactly rounded once, count int64 [nseg, nt], n int64 [nseg]): per segment
    the fraction of its columns that have each node type (types >= nt are counted nowhere; n = 1 for an empty one)."""
    nseg = len(seg_ptr) - 1
    cnt = np.zeros((nseg, nt), dtype=np.int64)
    n = np.ones(nseg, dtype=np.int64)
    for s in range(nseg):
        a, e = int(seg_ptr[s]), int(seg_ptr[s + 1])
        for p in range(a, e):
            ty = int(node_type[int(col[p])])
            if ty < nt:
                cnt[s, ty] += 1
        n[s] = max(e - a, 1)
    return cnt.astype(np.float64) / n[:, None].astype(np.float64), cnt, n


def expand(seg_ptr, col):
    """COO (row, col, dir) in CSR order (ofx_graph_expand)."""
    E = int(seg_ptr[-1])
    row, edir = np.empty(E, dtype=np.int64), np.empty(E, dtype=np.int64)
    for s in range(len(seg_ptr) - 1):
        for p in range(int(seg_ptr[s]), int(seg_ptr[s + 1])):
            row[p], edir[p] = s // 7, s % 7
    return row, np.asarray(col, dtype=np.int64).copy(), edir


def reverse(seg_ptr, col, n_nodes):
    """(rev_ptr [n * 7 + 1], rev_row [E], rev_w float32 [E]): forward edge (r, dir) -> c becomes an entry of reverse
    segment (c, dir) holding r with weight float32(1) / float32(size of the forward segment); every reverse segment in
    ascending row order (ofx_graph_reverse_count / _fill)."""
    buckets = [[] for _ in range(n_nodes * 7)]
    for s in range(n_nodes * 7):                                  # ascending s = ascending row per bucket
        a, e = int(seg_ptr[s]), int(seg_ptr[s + 1])
        for p in range(a, e):
            buckets[int(col[p]) * 7 + s % 7].append((s // 7, e - a))
    rev_ptr = exclusive_scan([len(b) for b in buckets])
    rows = np.array([r for b in buckets for r, _ in b], dtype=np.int64)
    size = np.array([n for b in buckets for _, n in b], dtype=np.float32)
    return rev_ptr, rows, (np.float32(1.0) / size).astype(np.float32) if size.size else size


# vectorised forms for CSRs with millions of segments (same results: tests/test_graph_oracle.py)
def primary_fast(seg_ptr, col):
    seg_ptr, col = np.asarray(seg_ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    n = seg_sizes(seg_ptr)
    first = col[np.minimum(seg_ptr[:-1], max(col.shape[0] - 1, 0))] if col.shape[0] else np.zeros_like(n)
    return np.where(n == 0, -1, np.where(n == 1, first, -2))


def primary_ext_fast(seg_ptr, col, n_src):
    seg_ptr = np.asarray(seg_ptr, dtype=np.int64)
    n = seg_sizes(seg_ptr)
    p = primary_fast(seg_ptr, col)
    rank = exclusive_scan(n > 1)
    return np.where(n == 0, n_src, np.where(n == 1, p, n_src + 1 + rank[:-1])), np.nonzero(n > 1)[0].astype(np.int64)


def type_frac_fast(seg_ptr, col, node_type, nt):
    seg_ptr, col = np.asarray(seg_ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    nseg = seg_ptr.shape[0] - 1
    n = seg_sizes(seg_ptr)
    seg_of = np.repeat(np.arange(nseg, dtype=np.int64), n)
    ty = np.asarray(node_type, dtype=np.int64)[col]
    keep = ty < nt
    cnt = np.bincount(seg_of[keep] * nt + ty[keep], minlength=nseg * nt).reshape(nseg, nt).astype(np.int64)
    n1 = np.maximum(n, 1)
    return cnt.astype(np.float64) / n1[:, None].astype(np.float64), cnt, n1


def expand_fast(seg_ptr, col):
    seg_ptr = np.asarray(seg_ptr, dtype=np.int64)
    seg_of = np.repeat(np.arange(seg_ptr.shape[0] - 1, dtype=np.int64), seg_sizes(seg_ptr))
    return seg_of // 7, np.asarray(col, dtype=np.int64).copy(), seg_of % 7


def reverse_fast(seg_ptr, col, n_nodes):
    seg_ptr, col = np.asarray(seg_ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    n = seg_sizes(seg_ptr)
    seg_of = np.repeat(np.arange(n_nodes * 7, dtype=np.int64), n)
    rkey = col * 7 + seg_of % 7
    order = np.lexsort((seg_of // 7, rkey))
    rev_ptr = exclusive_scan(np.bincount(rkey, minlength=n_nodes * 7))
    w = (np.float32(1.0) / n[seg_of].astype(np.float32)).astype(np.float32)
    return rev_ptr, (seg_of // 7)[order], w[order]


def _first_w(seg_ptr, w):
    seg_ptr, w = np.asarray(seg_ptr, dtype=np.int64), np.asarray(w, dtype=np.float32)
    return w[np.minimum(seg_ptr[:-1], max(w.shape[0] - 1, 0))] if w.shape[0] else np.zeros(seg_ptr.shape[0] - 1, np.float32)


def primary_w_fast(seg_ptr, col, w):
    n = seg_sizes(seg_ptr)
    p = primary_fast(seg_ptr, col)
    return np.where((n == 1) & (_first_w(seg_ptr, w) != np.float32(1.0)), -2, p)


def multi_flag_w_fast(seg_ptr, w):
    n = seg_sizes(seg_ptr)
    return ((n > 1) | ((n == 1) & (_first_w(seg_ptr, w) != np.float32(1.0)))).astype(np.int64)


def primary_ext_w_fast(seg_ptr, col, w, n_src):
    n = seg_sizes(seg_ptr)
    flag = multi_flag_w_fast(seg_ptr, w)
    rank = exclusive_scan(flag)
    p = primary_fast(seg_ptr, col)
    return (np.where(n == 0, n_src, np.where(flag == 1, n_src + 1 + rank[:-1], p)),
            np.nonzero(flag)[0].astype(np.int64))


def hand_csr(seed, n_nodes, nseg=None, n_src=None, sizes=(0, 1, 2, 255, 256, 1000)):
    """A CSR that is no tree: nseg (= 7 n_nodes) segments whose sizes are drawn from 0 / 1 / 2, with one segment each
    of 0, 1, 2, 255, 256 and 1000 entries planted; columns anywhere in [0, n_src) (= n_nodes).  (seg_ptr, col) int64."""
    g = np.random.default_rng(seed)
    nseg = n_nodes * 7 if nseg is None else nseg
    n_src = n_nodes if n_src is None else n_src
    if nseg == 0:
        return np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64)
    n = g.choice(np.array(sizes[:3]), size=nseg)
    for k, size in enumerate(sizes):                               # every size at least once (from six segments up)
        n[(k * nseg) // len(sizes)] = size
    seg_ptr = exclusive_scan(n)
    return seg_ptr, g.integers(0, n_src, size=int(seg_ptr[-1]))


def hand_weights(seed, n_edges):
    """float32 weights, three in four exactly 1: the others 0.25, 0.5 and the float32 just below 1"""
    g = np.random.default_rng(seed + 1000)
    pool = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 0.25, 0.5, np.nextafter(np.float32(1), np.float32(0))], dtype=np.float32)
    return pool[g.integers(0, pool.shape[0], size=n_edges)]


# ------------------------------------------------------------------------------------------------ node attributes
def leafrank(octree):
    """int64, all depths concatenated: per depth the exclusive count of leaves (children < 0) before each node
    (ofx_tree_leafrank)."""
    out = []
    for t in range(octree.depth + 1):
        rank, acc = [], 0
        for c in octree.children[t].tolist():
            rank.append(acc)
            acc += 1 if c < 0 else 0
        out.append(np.array(rank, dtype=np.int64))
    return np.concatenate(out)


def node_attributes(octree, d):
    """batch_id, node_type, keyd per graph row, and node_mask over [all nodes of fd..d-1 | nodes of d] -- its length is
    ncum[d] + nnum[d] - ncum[fd], NOT the number of rows (dual_octree.py:362-398)."""
    R = graph_rows(octree, d)
    fd = octree.full_depth
    mask = np.concatenate([(octree.children[t].numpy() < 0) for t in range(fd, d)] +
                          [np.ones(int(octree.nnum[d]), dtype=bool)])
    return dict(batch_id=R['b'], node_type=R['t'] - fd, keyd=R['key'] | (R['t'] << 58), node_mask=mask.astype(np.int64))


# ------------------------------------------------------------------------------------------------ the trees
TREES = ('deep_a', 'deep_b', 'deep_b_mid', 'deep_b_last', 'deep_c', 'full_face')
_RECIPES = {                                  # name: (B, full_depth, seed, p small, p large, empty element)
    'deep_a': (2, 2, 1, 0.25, 0.35, None),
    'deep_b': (3, 2, 2, 0.15, 0.5, 0),
    'deep_b_mid': (3, 2, 2, 0.15, 0.5, 1),
    'deep_b_last': (3, 2, 2, 0.15, 0.5, 2),
    'deep_c': (1, 3, 3, 0.05, 0.3, None),
}


def tree_splits(name):
    """(full_depth, small split [B, 8, S, S, S], large-split maker nnum -> [nnum, 8]) of a named tree."""
    import common as C
    if name == 'full_face':
        split = -torch.ones(2, 8, 4, 4, 4)
        split[0, :, 1, 2, 1] = 1.0                                 # an interior cell
        split[1, :, 0, 0, 3] = 1.0                                 # a corner cell
        return 2, split, lambda nnum: torch.ones(nnum, 8)
    B, fd, seed, ps, pl, empty = _RECIPES[name]
    split = C.random_split_small(B, fd, seed, p=ps)
    if empty is not None:
        split[empty] = -1.0                                        # an element with nothing below the full layer
    return fd, split, lambda nnum: C.random_split_large(nnum, seed + 10, p=pl)


def build_tree(name, sampler, device=None):
    """The named tree through `sampler`'s split2octree_small / split2octree_large (oracle.sampler on the host; the GPU
    tests pass the product's octree module and a device): a tree four levels deeper than its full layer."""
    fd, split, large = tree_splits(name)
    if device is not None:
        split = split.to(device)
    oc = sampler.split2octree_small(split, fd + 2, fd)
    ls = large(int(oc.nnum[fd + 2]))
    if device is not None:
        ls = ls.to(device)
    return sampler.split2octree_large(oc, ls, fd + 2)


@functools.lru_cache(maxsize=None)
def tree(name):
    """(oracle octree, OracleDualOctree after post-processing) of a named tree, built once per process."""
    from oracle import dual_octree as OD, sampler as OS
    oc = build_tree(name, OS)
    o_doc = OD.OracleDualOctree(oc)
    o_doc.post_processing_for_docnn()
    return oc, o_doc


@functools.lru_cache(maxsize=None)
def tree_csr(name, d):
    """(seg_ptr, col, N) of graph depth d of a named tree: from geometry where that is affordable, else from
    oracle/dual_octree.py (tests/test_graph_oracle.py shows the two equal wherever both run)."""
    oc, o_doc = tree(name)
    N = int(o_doc.graph[d]['node_type'].shape[0])
    seg_ptr, col = geometric_graph(oc, d) if N <= GEOMETRIC_MAX else csr_of_oracle(o_doc, d)
    return seg_ptr, col, N
