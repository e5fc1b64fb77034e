"""Float64 restatement of the NeuralMPU (csrc/ofx_graph.hip: ofx_mpu_eval, _eval_grid, _eval_grad, _backward) in plain
numpy.  TEST INFRASTRUCTURE: nothing here imports the product, nor oracle/mpu.py.

Written from the formulas in the header of oracle/mpu.py and the comment above MpuVisit in ofx_graph.hip.  Per query
point p = (x, y, z, batch), depth d in [ds, de] and each of the eight cell centres i around the point at that depth:

    X    = fl32(fl32(p + 1) * 2^(d-1)) - 0.5     the cell coordinate, ROUNDED TO FLOAT32 as the reference defines it
    f_i  = X - centre_i                           centre_i = floor(X) + (0|1 per axis), x slowest (mpu.py:37-52)
    w_i  = k_d prod_a (1 - |f_ia|)                k_d = float32(d * d / 50)
    v_i  = c_i . (f_i s_d) + c_i3                 s_d = 2 / 2^d, c_i = code[row_i]
    num  = sum w_i v_i,  den = sum w_i,  D = den + float32(1e-8),  sdf = num / D
    dw_ia = -sgn(f_ia) (2^d / 2) k_d prod_{b != a} (1 - |f_ib|)         sgn(0) = +1, floor detached (mpu.py:18-32)
    grad_a = (sum_i dw_ia v_i + w_i c_ia) / D - num (sum_i dw_ia) / D^2
    A_i  = a w_i / D + sum_a b_a (dw_ia / D - w_i dd_a / D^2)           a = dL/dsdf, b = dL/dgrad, dd_a = sum_i dw_ia
    dcode[row_i, a] += A_i f_ia s_d + b_a w_i / D,   dcode[row_i, 3] += A_i

over the centres that lie inside the cube, exist in the element trunc(p.w) of the tree and, below de, are leaves;
row_i = index inside depth d + nodes of depths ds .. d-1; mask = a centre of depth de exists.  Everything after X, k_d
and the 1e-8 is float64.

Node lookup is a sorted search on the oracle octree's KEYS (a node is a leaf when the key of its first child is absent
one depth down): the child pointers the kernel walks are never read.

Besides the values, `evaluate` returns the magnitudes the error bounds of tests/test_gpu_mpu_entry.py are written in:
S = sum w_i (|c_i0 f s| + |c_i1 f s| + |c_i2 f s| + |c_i3|), D, the sum of absolute values of every term of grad, and per
element of dcode the sum of absolute values of its contributions with their count m_row.

`mutant=` plants one of MUTANTS; tests/test_mpu_oracle.py shows that the bounds reject each of them.
"""
import numpy as np

U = 2.0 ** -24                               # unit roundoff of float32
EPS = float(np.float32(1e-8))
MUTANTS = ('kd_next', 'no_leaf_rule', 'sgn0', 'row_base_nempty', 'corner_flip')
COUNTS = (1, 7, 8, 33, 4099)                 # 8 n short of a wave, one wave exactly, past one block of 256 threads
CORNERS = np.array([[i >> 2 & 1, i >> 1 & 1, i & 1] for i in range(8)], dtype=np.int64)


def gamma(k):
    """k roundings of relative size <= 2^-24 compound to at most this relative error"""
    return k * U / (1.0 - k * U)


def k_sdf(nd):
    """Roundings on the way to sdf through nd depths, counted from the kernels (f s_d is exact: a power of two).
    v_i: 3 products + 3 additions feed |v| terms, at most 4 on one term.  w_i: three (1 - |f|) + three products = 6.
    w_i v_i: 1.  Accumulation over the depths: nd.  Three shuffle steps: 3.  So num carries 4 + 6 + 1 + nd + 3 = 14 + nd
    relative to S, and D carries 6 + nd + 3 + 1 (the + eps) = 10 + nd.  ofx_mpu_eval divides (1); ofx_mpu_eval_grad
    forms 1 / D and multiplies (2).  |sdf| <= S / D, so K = (14 + nd) + (10 + nd) + 2 = 26 + 2 nd."""
    return 26 + 2 * nd


def k_grad(nd):
    """dw_ia: (1 - |f|) twice, their product, half * k_d, the product with it = 5.  dw v: 5 + 4 + 1 = 10; w c: 6 + 1;
    their sum 1; accumulation nd + 3: dn carries 14 + nd, dd carries 5 + nd + 3 = 8 + nd.  1 / D carries 11 + nd.
    dn / D: (14 + nd) + (11 + nd) + 1 = 26 + 2 nd.  r = num / D / D: (14 + nd) + 2 (11 + nd) + 2 = 38 + 3 nd; r dd:
    + (8 + nd) + 1 = 47 + 4 nd.  The final subtraction: 1.  K = 48 + 4 nd on the sum of absolute values of all terms."""
    return 48 + 4 * nd


def k_dcode(nd):
    """One contribution: w / D = 6 + (11 + nd) + 1 = 18 + nd; a w / D: 19 + nd.  b (dw - (w / D) dd) / D: the inner product
    (18 + nd) + (8 + nd) + 1 = 27 + 2 nd, the subtraction 1, the 1 / D product (11 + nd) + 1, the b product 1 = 41 + 3 nd.
    The four terms of A_i add in 3 steps: 44 + 3 nd.  A f s: 1, + b w / D: 1.  K = 46 + 3 nd; the m_row atomic additions
    into the element come on top, in any order."""
    return 46 + 3 * nd


# ------------------------------------------------------------------------------------------------ the tree, by its keys
def morton(x, y, z, depth):
    """level bit i of x -> key bit 3 i + 2, y -> 3 i + 1, z -> 3 i"""
    x, y, z = (np.asarray(v, dtype=np.int64) for v in (x, y, z))
    key = np.zeros_like(x)
    for i in range(depth):
        key |= ((x >> i) & 1) << (3 * i + 2) | ((y >> i) & 1) << (3 * i + 1) | ((z >> i) & 1) << (3 * i)
    return key


def unmorton(key, depth):
    key = np.asarray(key, dtype=np.int64)
    b, k = key >> 48, key & ((1 << 48) - 1)
    x, y, z = np.zeros_like(k), np.zeros_like(k), np.zeros_like(k)
    for i in range(depth):
        x |= ((k >> (3 * i + 2)) & 1) << i
        y |= ((k >> (3 * i + 1)) & 1) << i
        z |= ((k >> (3 * i)) & 1) << i
    return x, y, z, b


class KeyTree:
    """The sorted keys of every depth of an oracle octree (anything with .keys, .nnum, .nnum_nempty, .depth,
    .full_depth, .batch_size)."""

    def __init__(self, oc):
        self.depth, self.full_depth, self.batch_size = int(oc.depth), int(oc.full_depth), int(oc.batch_size)
        self.keys = [np.asarray(oc.keys[d].numpy() if hasattr(oc.keys[d], 'numpy') else oc.keys[d], dtype=np.int64)
                     for d in range(self.depth + 1)]
        self.nnum = [int(oc.nnum[d]) for d in range(self.depth + 1)]
        self.nnum_nempty = [int(oc.nnum_nempty[d]) for d in range(self.depth + 1)]
        for d, k in enumerate(self.keys):
            assert k.shape[0] == self.nnum[d] and np.all(k[1:] > k[:-1]), 'keys of depth %d are not sorted' % d

    def find(self, key, d):
        """index of each key among the keys of depth d, -1 where absent"""
        keys = self.keys[d]
        key = np.asarray(key, dtype=np.int64)
        pos = np.searchsorted(keys, key)
        hit = np.zeros(key.shape, dtype=bool)
        ok = pos < keys.shape[0]
        hit[ok] = keys[pos[ok]] == key[ok]
        return np.where(hit, pos, -1)

    def is_leaf(self, key, d):
        """no child one depth down (every node of the deepest level counts as a leaf)"""
        if d >= self.depth:
            return np.ones(np.shape(key), dtype=bool)
        key = np.asarray(key, dtype=np.int64)
        first = ((key & ((1 << 48) - 1)) << 3) | (key >> 48 << 48)
        return self.find(first, d + 1) < 0

    def rows(self, ds, de):
        return sum(self.nnum[ds:de + 1])


def cell_coord(p32, d):
    """fl32(fl32(p + 1) * 2^(d-1)) - 0.5 in float32, widened"""
    p32 = np.asarray(p32, dtype=np.float32)
    t = (p32 + np.float32(1.0)).astype(np.float32)
    x = (t * np.float32(2.0 ** (d - 1))).astype(np.float32) - np.float32(0.5)
    assert x.dtype == np.float32
    return x.astype(np.float64)


def batch_of(pts32):
    return np.trunc(np.asarray(pts32, dtype=np.float32)[:, 3]).astype(np.int64)


def visit(T, d, de, pts32, mutant=None):
    """Per (point, corner) of depth d: idx (-1: outside, absent or wrong element), use, f [n, 8, 3] float64."""
    X = cell_coord(pts32[:, :3], d)
    base = np.floor(X)
    centre = base[:, None, :] + CORNERS[None].astype(np.float64)
    f = X[:, None, :] - centre
    if mutant == 'corner_flip':                                   # corner 5's x offset from the other side
        f = f.copy()
        f[:, 5, 0] = X[:, 0] - base[:, 0]
    c = centre.astype(np.int64)
    b = np.broadcast_to(batch_of(pts32)[:, None], c.shape[:2])
    inb = np.all((c >= 0) & (c < (1 << d)), axis=-1) & (b >= 0) & (b < T.batch_size)
    cc = np.where(inb[..., None], c, 0)
    key = morton(cc[..., 0], cc[..., 1], cc[..., 2], d) | (np.where(inb, b, 0) << 48)
    idx = np.where(inb, T.find(key, d), -1)
    found = idx >= 0
    use = found.copy()
    if d < de and mutant != 'no_leaf_rule':
        use &= T.is_leaf(key, d)
    return idx, found, use, f


def evaluate(T, ds, de, pts32, code, dsdf=None, dgrad=None, dcode0=None, mutant=None):
    """All outputs of the four entry points and the magnitudes of their bounds, float64.
    pts32 float32 [n, 4]; code [rows, 4]; dsdf [n] / dgrad [n, 3] (None = zeros); dcode0 = the table accumulated into."""
    assert 0 <= ds <= de <= T.depth
    pts32 = np.asarray(pts32, dtype=np.float32).reshape(-1, 4)
    code = np.asarray(code, dtype=np.float64)
    n, rows = pts32.shape[0], T.rows(ds, de)
    assert code.shape == (rows, 4)
    a = np.zeros(n) if dsdf is None else np.asarray(dsdf, dtype=np.float64)
    bk = np.zeros((n, 3)) if dgrad is None else np.asarray(dgrad, dtype=np.float64)
    num, den, S = np.zeros(n), np.zeros(n), np.zeros(n)
    dn, dd, dnabs, ddabs = (np.zeros((n, 3)) for _ in range(4))
    mask = np.zeros(n, dtype=bool)
    used = np.zeros(n, dtype=np.int64)                            # centres that contribute (some with weight 0)
    per_depth = []
    row_base = 0
    for d in range(ds, de + 1):
        idx, found, use, f = visit(T, d, de, pts32, mutant)
        if d == de:
            mask = found.any(-1)
        used += use.sum(-1)
        kd = float(np.float32((d + 1) ** 2 / 50.0 if mutant == 'kd_next' else d * d / 50.0))
        s, half = 2.0 / 2 ** d, 2 ** d / 2.0
        row = np.where(use, idx + row_base, 0)
        c = np.where(use[..., None], code[row], 0.0)               # [n, 8, 4]
        om = 1.0 - np.abs(f)                                       # [n, 8, 3]
        u = use.astype(np.float64)
        w = kd * om.prod(-1) * u
        fs = f * s
        v = (c[..., :3] * fs).sum(-1) + c[..., 3]
        vabs = np.abs(c[..., :3] * fs).sum(-1) + np.abs(c[..., 3])
        sg = np.where(f < 0, -1.0, 1.0)
        if mutant == 'sgn0':
            sg = np.sign(f)
        others = np.stack([om[..., 1] * om[..., 2], om[..., 0] * om[..., 2], om[..., 0] * om[..., 1]], -1)
        dw = -sg * (half * kd) * others * u[..., None]
        num += (w * v).sum(-1)
        den += w.sum(-1)
        S += (w * vabs).sum(-1)
        dn += (dw * v[..., None] + w[..., None] * c[..., :3]).sum(1)
        dnabs += (np.abs(dw) * vabs[..., None] + w[..., None] * np.abs(c[..., :3])).sum(1)
        dd += dw.sum(1)
        ddabs += np.abs(dw).sum(1)
        per_depth.append((use, row, w, dw, fs))
        row_base += T.nnum_nempty[d] if mutant == 'row_base_nempty' else T.nnum[d]
    D = den + EPS
    sdf = num / D
    grad = dn / D[:, None] - (num / D ** 2)[:, None] * dd
    gabs = dnabs / D[:, None] + (S / D ** 2)[:, None] * ddabs
    # the adjoint w.r.t. the code table
    dcode = np.zeros((rows, 4)) if dcode0 is None else np.array(dcode0, dtype=np.float64)
    dabs = np.abs(dcode)
    m_row = np.zeros(rows, dtype=np.int64)
    Dc, ac, bc = D[:, None], a[:, None], bk[:, None, :]
    for use, row, w, dw, fs in per_depth:
        wD = w / Dc
        A = ac * wD + (bc * (dw / Dc[..., None] - (wD / Dc)[..., None] * dd[:, None, :])).sum(-1)
        Aabs = np.abs(ac) * wD + (np.abs(bc) * (np.abs(dw) / Dc[..., None] +
                                                (wD / Dc)[..., None] * ddabs[:, None, :])).sum(-1)
        con = np.concatenate([A[..., None] * fs + bc * wD[..., None], A[..., None]], -1)
        cab = np.concatenate([Aabs[..., None] * np.abs(fs) + np.abs(bc) * wD[..., None], Aabs[..., None]], -1)
        r = row[use]
        np.add.at(dcode, r, con[use])
        np.add.at(dabs, r, cab[use])
        np.add.at(m_row, r, 1)
    return dict(sdf=sdf, mask=mask, grad=grad, S=S, D=D, gabs=gabs, dcode=dcode, dabs=dabs, m_row=m_row, den=den,
                used=used)


def bounds(R, nd):
    """(sdf, grad, dcode) elementwise bounds of a result of `evaluate` over nd depths."""
    return (gamma(k_sdf(nd)) * R['S'] / R['D'], gamma(k_grad(nd)) * R['gabs'],
            (k_dcode(nd) + R['m_row'])[:, None] * U / (1.0 - (k_dcode(nd) + R['m_row'])[:, None] * U) * R['dabs'])


# ------------------------------------------------------------------------------------------------ inputs
def ranges(T):
    """The depth ranges (ds, de) the tests run."""
    fd, dp = T.full_depth, T.depth
    return [(fd, dp), (fd, fd), (fd + 1, dp), (dp, dp), (0, fd + 1)]


def lattice(size, step, bbmin, batch, head=0, count=None):
    """Points head .. head + count of the size^3 lattice of ofx_mpu_eval_grid, x slowest: fl32(fl32(i * step) + bbmin)."""
    ax = np.arange(size, dtype=np.float32) * np.float32(step) + np.float32(bbmin)
    assert ax.dtype == np.float32
    pts = np.stack(np.meshgrid(ax, ax, ax, indexing='ij'), -1).reshape(-1, 3)
    pts = np.concatenate([pts, np.full((pts.shape[0], 1), batch, dtype=np.float32)], 1).astype(np.float32)
    count = pts.shape[0] - head if count is None else count
    return np.ascontiguousarray(pts[head:head + count])


def empty_elements(T):
    """batch elements with no node below the full layer"""
    if T.depth == T.full_depth:
        return []
    have = set((T.keys[T.full_depth + 1] >> 48).tolist())
    return [b for b in range(T.batch_size) if b not in have]


def _to_p(cell, d):
    """cell coordinate X -> p with fl32(fl32(p + 1) * 2^(d-1)) - 0.5 == X whenever (X + 0.5) / 2^(d-1) is a float32"""
    return (cell + 0.5) / 2.0 ** (d - 1) - 1.0


def points(T, ds, de, n, seed=0):
    """(pts float32 [n, 4], kind int [n]): the first 5/8 of the points (rounded up) are jittered centres of existing
    nodes of depth de (their mask is 1), the rest go round the other kinds in turn:
      0 jittered centre of a node of depth de     1 jittered centre of a node of another depth of the range
      2 on a cell-centre plane (one to three axes) of a depth of the range    3 on a cell face of a depth of the range
      4 on a face of the cube    5 just outside the cube    6 inside a region whose depth-de cell is absent
      7 in an empty batch element (trees that have one; otherwise kind 6); 6 and 7 turn into 0 when de is a full layer
      8 batch id -1, B or B + 3    9 fractional batch id 0.5 or B - 0.001 at a jittered centre."""
    g = np.random.default_rng(1000 * seed + 17 * ds + de)
    B = T.batch_size
    pts = np.zeros((n, 4), dtype=np.float64)
    kind = np.zeros(n, dtype=np.int64)
    n0 = (5 * n + 7) // 8
    empties = empty_elements(T)

    def node_centre(d, jitter, element=None):
        m = np.arange(T.nnum[d]) if element is None else np.nonzero((T.keys[d] >> 48) == element)[0]
        if m.size == 0:
            m = np.arange(T.nnum[d])
        i = int(m[int(g.integers(0, m.size))])
        x, y, z, b = unmorton(T.keys[d][i:i + 1], d)
        c = np.array([x[0], y[0], z[0]], dtype=np.float64)
        return _to_p(c + g.uniform(-jitter, jitter, 3), d), float(b[0])

    for i in range(n):
        k = 0 if i < n0 else 1 + (i - n0) % 9
        d = int(g.integers(ds, de + 1))
        if k == 0:
            p, b = node_centre(de, 0.49)
        elif k == 1:
            p, b = node_centre(d, 0.49)
        elif k in (2, 3):
            p, b = node_centre(d if i % 2 else de, 0.49)
            axes = g.permutation(3)[:int(g.integers(1, 4))]
            cell = np.floor((p + 1.0) * 2.0 ** (d - 1) - 0.5)
            on = cell + (0.0 if k == 2 else 0.5) + g.integers(0, 2, 3)
            p[axes] = _to_p(on, d)[axes]
        elif k == 4:
            p, b = node_centre(de, 0.49)
            ax = int(g.integers(0, 3))
            p[ax] = (-1.0, 1.0)[int(g.integers(0, 2))]
            if i % 3 == 0:
                p[:] = np.where(g.integers(0, 2, 3) > 0, 1.0, -1.0)   # a corner of the cube
        elif k == 5:
            p, b = node_centre(de, 0.49)
            ax = int(g.integers(0, 3))
            out = [np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(-1), np.float32(-2)),
                   np.float32(1.0) + np.float32(2.0 ** -de), np.float32(-1.0) - np.float32(2.0 ** -de), 1.09, -1.09]
            p[ax] = float(out[int(g.integers(0, len(out)))])
        elif k in (6, 7) and de <= T.full_depth:
            k = 0                                                  # a full layer has neither absent cells nor empty elements
            p, b = node_centre(de, 0.49)
        elif k == 6 or (k == 7 and not empties):
            k = 6
            nb = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing='ij'), -1).reshape(-1, 3)
            for _ in range(256):                                   # a cell none of whose 27 neighbours exists
                c = g.integers(0, 1 << de, 3)
                b = float(g.integers(0, B))
                q = c[None] + nb
                q = q[np.all((q >= 0) & (q < (1 << de)), axis=1)]
                if np.all(T.find(morton(q[:, 0], q[:, 1], q[:, 2], de) | (int(b) << 48), de) < 0):
                    break
            else:
                raise AssertionError('no absent region at depth %d' % de)
            p = _to_p(c + g.uniform(-0.49, 0.49, 3), de)
        elif k == 7:
            p, _ = node_centre(de, 0.49)
            b = float(empties[int(g.integers(0, len(empties)))])
        elif k == 8:
            p, _ = node_centre(de, 0.49)
            b = float((-1, B, B + 3)[(i - n0) // 9 % 3])
        elif (i - n0) // 9 % 2 == 0:
            p, _ = node_centre(de, 0.49, element=0)
            b = 0.5                                                # truncates to element 0
        else:
            p, _ = node_centre(de, 0.49, element=B - 1)
            b = B - 0.001                                          # truncates to element B - 1
        pts[i, :3], pts[i, 3], kind[i] = p, b, k
    return pts.astype(np.float32), kind


def code_table(T, ds, de, seed=0):
    """float32 codes of size O(1), every row different"""
    g = np.random.default_rng(7 + seed)
    return g.standard_normal((T.rows(ds, de), 4)).astype(np.float32)
