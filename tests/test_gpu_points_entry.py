"""The point-cloud kernels (csrc/ofx_points.hip) one entry point at a time through the C ABI, against
tests/train_oracle.py.  Integer outputs are compared bit for bit; every output, and the sort workspace (sized exactly
ofx_points_sort_ws_bytes(n)), sits between sentinel bands that must come back untouched.

    entry point                   cases                                                          refusals (OFX_EINVAL)
    ofx_points_keys               test_keys: n = 0, 1, 257, 2 097 152 + 300 (the grid-stride      n < 0, depth 0 / 17, ldp 2,
                                  step); depth 1, 6, 16; ldp 3, 7; batch ids up to 32 767, and    batch_const -1, NULL pts / keys /
                                  NULL with batch_const 5; coordinates on and one ulp off both    idx with n > 0
                                  cube faces, outside the cube, on and one ulp below cell faces
    ofx_points_sort               test_sort: n = 0, 1, 2, 255, 256, 257, 65 537, 2 097 152 + 300;  ws_bytes one short, each NULL,
                                  few distinct keys using bits 0..62, idx_in descending           n < 0, n > 2^30
    ofx_octree_label_from_points  test_label_edges (d = 0, depth_pts and between: a point in the  d > depth_pts, depth_pts > 16,
                                  first / last finest cell of a node, of its neighbours, the      d < 0, n_pts < 0, nnum < 0, NULL
                                  same code under another batch id; depth_pts = 16 at d = 0),     node_keys / label with nnum > 0,
                                  test_label_random (nnum = 2 097 152 + 300), n_pts = 0           NULL sorted_keys with n_pts > 0
    ofx_octree_point_features     test_features: nodes of 0, 1, 2 and 1000 points, normals that   n_pts < 0, nnum < 0, depth 0 / 17,
                                  cancel, ldp 5 / ldn 4, NULL normals / feat / avg_points /       ldp 2, ldn 2 with normals, NULL
                                  avg_normals, nnum = 2 097 152 + 300 with the filled nodes last  node_keys, NULL sorted_keys / idx
                                                                                                  / pts with n_pts > 0, feat 4
                                                                                                  bytes off 16

The features' coordinates lie on the grid j / 2^10 inside their cell and the normals on k / 2^10: every fp32 sum is
exact (asserted on the reference) and every average stays 2^-10 away from a cell face, where frac() jumps -- that jump
is not under test.  avg_points within 2 U of its value, the normal and the dot product through glue_oracle.assert_close
with the constants POINTS_C_* counted in train_oracle.
"""
import numpy as np
import pytest
import torch

import train_oracle as T
from glue_oracle import assert_close
from test_gpu_graph_tables import Guarded, _p, _up
from test_gpu_loss_entry import Window, _bits, _call, _refused

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

BIG = T.GRID_CAP + 300


def _settled(*guards):
    torch.cuda.synchronize()
    for g in guards:
        assert g.untouched()


# ------------------------------------------------------------------------------------------------ ofx_points_keys
def _coordinates(n, depth, seed):
    """[n, 3] float32 in [-1.2, 1.2] with, in front and rotating through x, y, z: -1, one ulp below it, -1.5,
    nextafter(1, 0) -- p + 1 rounds to 2.0: the clamp acts on a point Points.clip keeps --, 1, 1.5, +-3 (at depth 1
    nothing nearer truncates below 0), and cell faces k / 2^(depth-1) - 1 with the value one ulp below each"""
    g = np.random.default_rng(seed)
    pts = g.uniform(-1.2, 1.2, size=(n, 3)).astype(np.float32)
    f = np.float32
    sp = [f(-1), np.nextafter(f(-1), f(-2)), f(-1.5), np.nextafter(f(1), f(0)), f(1), f(1.5), f(-3), f(3)]
    for k in sorted({1, 2, 2 ** (depth - 1), 2 ** depth - 1, 2 ** depth // 3 + 1} & set(range(1, 2 ** depth))):
        face = f(k / 2.0 ** (depth - 1) - 1.0)
        sp += [face, np.nextafter(face, f(-2))]
    m = min(n, 3 * len(sp))
    for i in range(m):
        pts[i, i % 3] = sp[i // 3]
    return pts


@pytest.mark.parametrize('n,depth,ldp,const', [(0, 6, 3, False), (1, 1, 3, True), (1, 16, 7, False), (257, 1, 7, False),
                                                (257, 6, 3, True), (257, 6, 7, False), (257, 16, 3, False),
                                                (BIG, 16, 7, False), (BIG, 1, 3, True)])
def test_keys(n, depth, ldp, const):
    pts = _coordinates(n, depth, 10 * depth + ldp)
    pw = Window(n, 3, ldp, ldp - 3, pts)
    batch = np.random.default_rng(n + depth).integers(0, 32768, size=n)
    if n:
        batch[0], batch[-1] = 32767, 0
    bd = _up(batch, torch.int32)
    keys, idx = Guarded(n, torch.int64), Guarded(n, torch.int32)
    _call('ofx_points_keys', pw.ptr, ldp, None if const else _p(bd), 5 if const else 0, n, depth, keys.ptr, idx.ptr)
    want = T.points_keys(pts, 5 if const else batch, depth)
    assert np.array_equal(keys.get(), want)
    assert np.array_equal(idx.get(), np.arange(n))
    if n >= 257:                                                   # the clamp acted on both faces, in the oracle too
        q = np.trunc(T.scaled(pts, depth))
        assert (q < 0).any() and (q > 2 ** depth - 1).any() and np.all(want >= 0)
        assert T.scaled(np.array([[np.nextafter(np.float32(1), np.float32(0))] * 3]), depth)[0, 0] == 2.0 ** depth


def test_keys_refusals():
    pw = Window(8, 3, 3, 0, np.zeros((8, 3), np.float32))
    keys, idx = Guarded(8, torch.int64), Guarded(8, torch.int32)
    ok = dict(pts=pw.ptr, ldp=3, const=0, n=8, depth=6, keys=keys.ptr, idx=idx.ptr)
    for bad in (dict(n=-1), dict(depth=0), dict(depth=17), dict(ldp=2), dict(const=-1), dict(pts=None), dict(keys=None),
                dict(idx=None)):
        a = dict(ok, **bad)
        _refused('ofx_points_keys', a['pts'], a['ldp'], None, a['const'], a['n'], a['depth'], a['keys'], a['idx'])
    _call('ofx_points_keys', None, 3, None, 0, 0, 6, None, None)                   # nothing to read or write
    _settled(keys, idx)


# ------------------------------------------------------------------------------------------------ ofx_points_sort
def _ws(n):
    from octfusion_amd import _lib
    nbytes = int(_lib.lib().ofx_points_sort_ws_bytes(n))
    assert nbytes >= 16
    return Guarded(nbytes, torch.uint8), nbytes


def _sort_keys(n, seed):
    """few distinct keys (about n / 20, at most 37): batch ids up to 32 767 in bits 48..62 over 48-bit codes"""
    g = np.random.default_rng(seed)
    distinct = (g.integers(0, 32768, size=37) << 48) | g.integers(0, 2 ** 48, size=37)
    distinct[:3] = [0, (32767 << 48) | (2 ** 48 - 1), 1 << 48]
    return distinct[g.integers(0, max(1, min(37, n // 20 + 1)), size=n)]


@pytest.mark.parametrize('n', [0, 1, 2, 255, 256, 257, 65537, BIG])
def test_sort(n):
    keys = _sort_keys(n, n)
    idx = np.arange(n)[::-1].copy()
    kd, idd = _up(keys, torch.int64), _up(idx, torch.int32)
    ko, io = Guarded(n, torch.int64), Guarded(n, torch.int32)
    ws, nbytes = _ws(n)
    _call('ofx_points_sort', _p(kd), _p(idd), n, ko.ptr, io.ptr, ws.ptr, nbytes)
    wk, wi = T.points_sort(keys, idx)
    assert np.array_equal(ko.get(), wk) and np.array_equal(io.get(), wi)
    assert ws.bands_intact()
    if n > 1:                                                      # stable: inside a run of equal keys, the input order
        same = wk[1:] == wk[:-1]
        assert same.any() and np.all(io.get()[1:][same] < io.get()[:-1][same])
    assert np.array_equal(kd[0].cpu().numpy(), keys) and np.array_equal(idd[0].cpu().numpy(), idx)       # inputs intact
    if n == 0:
        _call('ofx_points_sort', None, None, 0, None, None, None, 0)


def test_sort_refusals():
    n = 100
    kd, idd = _up(_sort_keys(n, 1), torch.int64), _up(np.arange(n), torch.int32)
    ko, io = Guarded(n, torch.int64), Guarded(n, torch.int32)
    ws, nbytes = _ws(n)
    ok = dict(k=_p(kd), i=_p(idd), n=n, ko=ko.ptr, io=io.ptr, ws=ws.ptr, b=nbytes)
    for bad in (dict(b=nbytes - 1), dict(k=None), dict(i=None), dict(ko=None), dict(io=None), dict(ws=None), dict(n=-1),
                dict(n=2 ** 30 + 1)):
        a = dict(ok, **bad)
        _refused('ofx_points_sort', a['k'], a['i'], a['n'], a['ko'], a['io'], a['ws'], a['b'])
    _settled(ko, io, ws)


# ------------------------------------------------------------------------------------------------ label_from_points
def _label(sorted_keys, node_keys, depth_pts, d, null_keys=False):
    sk, nk = _up(sorted_keys, torch.int64), _up(node_keys, torch.int64)
    label = Guarded(len(node_keys), torch.int32)
    _call('ofx_octree_label_from_points', None if null_keys else _p(sk), len(sorted_keys), _p(nk), len(node_keys),
          depth_pts, d, label.ptr)
    got = label.get()
    assert np.array_equal(got, T.label_from_points(sorted_keys, node_keys, depth_pts, d))
    return got


def test_label_edges():
    """depth_pts = 6.  Batch 2 holds a point in the FIRST finest cell of depth-3 node 10, one in the LAST of node 12, one
    in the last of node 19 and one in the first of node 22; batch 5 one inside node 30."""
    B = lambda b: b << 48
    pts = np.array(sorted([B(2) | (10 << 9), B(2) | (12 << 9) | 511, B(2) | ((20 << 9) - 1), B(2) | (22 << 9),
                           B(5) | (30 << 9) | 7]), dtype=np.int64)
    nodes = [(2, 9), (2, 10), (2, 11), (2, 12), (2, 13), (2, 19), (2, 20), (2, 21), (2, 22), (2, 23), (2, 30), (5, 30),
             (4, 30), (0, 10), (6, 0), (5, 29), (5, 31)]
    want = [0, 1, 0, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0]
    got = _label(pts, np.array([B(b) | m for b, m in nodes], dtype=np.int64), 6, 3)
    assert got.tolist() == want
    # d = depth_pts: the span is one key
    fine = np.array([pts[0] - 1, pts[0], pts[0] + 1, pts[1] - 1, pts[1], pts[1] + 1, pts[4], pts[4] ^ B(5) ^ B(4)], dtype=np.int64)
    assert _label(pts, fine, 6, 6).tolist() == [0, 1, 0, 0, 1, 0, 1, 0]
    # d = 0: the whole element; ids before, between and after those that hold points
    roots = np.array([B(b) for b in (0, 1, 2, 3, 4, 5, 6, 32767)], dtype=np.int64)
    assert _label(pts, roots, 6, 0).tolist() == [0, 0, 1, 0, 0, 1, 0, 0]
    # depth_pts = 16 at d = 0: a shift of 48 bits; the first and the last code of an element
    deep = np.array([B(1), B(3) | (2 ** 48 - 1)], dtype=np.int64)
    assert _label(deep, roots, 16, 0).tolist() == [0, 1, 0, 1, 0, 0, 0, 0]
    assert _label(deep, np.array([B(1) | 0, B(1) | 1, B(3) | (8 ** 15 - 1), B(3) | (8 ** 15 - 2), B(2) | (8 ** 15 - 1)],
                                 dtype=np.int64), 16, 15).tolist() == [1, 0, 1, 0, 0]
    # no points: every label 0, sorted_keys may be NULL
    assert not _label(np.zeros(0, np.int64), roots, 6, 0, null_keys=True).any()
    assert not _label(np.zeros(0, np.int64), roots, 6, 0).any()


@pytest.mark.parametrize('nnum,d', [(0, 3), (1, 3), (257, 2), (BIG, 3), (4099, 6)])
def test_label_random(nnum, d):
    g = np.random.default_rng(nnum + d)
    pts = np.sort((g.choice([0, 2, 5], size=3000) << 48) | g.integers(0, 8 ** 6, size=3000)).astype(np.int64)
    nodes = (g.choice([0, 1, 2, 5, 6], size=nnum) << 48) | g.integers(0, 8 ** d, size=nnum)
    pick = g.integers(0, len(pts), size=nnum // 2)                 # half the nodes next to a point: its cell, the one
    near = ((pts[pick] & (2 ** 48 - 1)) >> (3 * (6 - d))) + g.integers(-1, 2, size=len(pick))      # before, the one after
    nodes[:len(pick)] = (pts[pick] >> 48 << 48) | np.clip(near, 0, 8 ** d - 1)
    got = _label(pts, nodes.astype(np.int64), 6, d)
    if nnum > 256:
        assert 0 < got.sum() < nnum


def test_label_refusals():
    sk, nk = _up(np.arange(4), torch.int64), _up(np.arange(4), torch.int64)
    label = Guarded(4, torch.int32)
    ok = dict(sk=_p(sk), n_pts=4, nk=_p(nk), nnum=4, depth=6, d=3, label=label.ptr)
    for bad in (dict(d=7), dict(depth=17, d=17), dict(depth=17), dict(d=-1), dict(n_pts=-1), dict(nnum=-1), dict(nk=None),
                dict(label=None), dict(sk=None)):
        a = dict(ok, **bad)
        _refused('ofx_octree_label_from_points', a['sk'], a['n_pts'], a['nk'], a['nnum'], a['depth'], a['d'], a['label'])
    _call('ofx_octree_label_from_points', _p(sk), 4, None, 0, 6, 3, None)          # no nodes: nothing to read or write
    _settled(label)


# ------------------------------------------------------------------------------------------------ point_features
DEPTH = 6


def _feature_case(nnum, seed):
    """nnum nodes of depth 6 in elements 0 and 3; all but the last seven are empty (the filled ones come last: past the
    grid-stride step when nnum is large).  The filled ones hold 1, 2, 1000, 2 (normals that cancel), 1, 2 and 5 points;
    the 1000-point node sits at a cell with coordinates < 16 so that its fp32 sums stay exact."""
    g = np.random.default_rng(seed)
    counts = [1, 2, 1000, 2, 1, 2, 5]
    cells = np.concatenate([g.integers(0, 64, size=(2, 3)), [[15, 7, 11]], g.integers(0, 64, size=(4, 3))])
    batch = np.array([0, 0, 0, 3, 3, 3, 3])
    filled = (batch << 48) | T.morton(cells[:, 0], cells[:, 1], cells[:, 2])
    assert len(set(filled.tolist())) == 7
    empty = (g.choice([1, 2, 4], size=max(nnum - 7, 0)) << 48) | g.integers(0, 8 ** DEPTH, size=max(nnum - 7, 0))
    node_keys = np.concatenate([empty, filled[:nnum]]).astype(np.int64)
    pts, nrm, pb = [], [], []
    for j, c in enumerate(counts[:nnum]):
        q = cells[j] + g.integers(1, 1024, size=(c, 3)) / 1024.0                   # scaled position, 10 fraction bits
        pts.append(q / 2.0 ** (DEPTH - 1) - 1.0)
        v = g.integers(-1024, 1025, size=(c, 3)) / 1024.0
        if j == 3:
            v[1] = -v[0]
        nrm.append(v)
        pb.append(np.full(c, batch[j]))
    pts, nrm, pb = np.concatenate(pts), np.concatenate(nrm), np.concatenate(pb)
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
    perm = g.permutation(len(pts))
    pts, nrm, pb = pts[perm].astype(np.float32), nrm[perm].astype(np.float32), pb[perm]
    sk, si = T.points_sort(T.points_keys(pts, pb, DEPTH), np.arange(len(pts)))
    return node_keys, pts, nrm, sk, si


@pytest.mark.parametrize('nnum', [7, 300, BIG])
def test_features(nnum):
    node_keys, pts, nrm, sk, si = _feature_case(nnum, nnum)
    n = len(pts)
    pw, nw = Window(n, 3, 5, 1, pts), Window(n, 3, 4, 0, nrm)
    skd, sid, nkd = _up(sk, torch.int64), _up(si, torch.int32), _up(node_keys, torch.int64)
    for variant in ('all', 'no normals', 'no feat', 'no avg_points', 'no avg_normals'):
        normals = None if variant == 'no normals' else nrm
        feat, ap, an = Guarded(4 * nnum, torch.float32), Guarded(3 * nnum, torch.float32), Guarded(3 * nnum, torch.float32)
        assert feat.ptr % 16 == 0
        _call('ofx_octree_point_features', _p(skd), _p(sid), n, pw.ptr, 5, None if normals is None else nw.ptr, 4, _p(nkd),
              nnum, DEPTH, None if variant == 'no feat' else feat.ptr, None if variant == 'no avg_points' else ap.ptr,
              None if variant == 'no avg_normals' else an.ptr)
        rf, ra, rn, S_dot, exact = T.point_features(sk, si, pts, normals, node_keys, DEPTH)
        assert exact
        full = np.abs(ra).sum(1) > 0
        assert full.sum() == 7 and np.all(np.minimum(ra[full] % 1.0, 1.0 - ra[full] % 1.0) >= 2.0 ** -10)
        if variant == 'no feat':
            assert feat.untouched()
        else:
            f = feat.get().reshape(nnum, 4)
            assert np.all(_bits(f[~full]) == 0)
            u1 = assert_close(torch.tensor(f[:, :3]), torch.tensor(rf[:, :3]), np.abs(rf[:, :3]), T.POINTS_C_NORMAL, 'normal')
            u2 = assert_close(torch.tensor(f[:, 3]), torch.tensor(rf[:, 3]), S_dot, T.POINTS_C_DOT, 'dot')
            print('features nnum %d %s: the normal uses %.3f, the dot product %.3f of the bound' % (nnum, variant, u1, u2))
            zero = full & (np.abs(rn).sum(1) == 0)                 # cancelled (or absent) normals: a zero normal, not NaN
            assert zero.sum() == (7 if normals is None else 1) and np.all(f[zero] == 0)
            if variant != 'no avg_normals':
                assert np.array_equal(_bits(an.get().reshape(nnum, 3)), _bits(f[:, :3]))
        if variant == 'no avg_points':
            assert ap.untouched()
        else:
            u = assert_close(torch.tensor(ap.get().reshape(nnum, 3)), torch.tensor(ra), np.abs(ra), T.POINTS_C_AVG, 'avg_points')
            assert np.all(_bits(ap.get().reshape(nnum, 3)[~full]) == 0)
            print('features nnum %d %s: avg_points uses %.3f of the bound' % (nnum, variant, u))
        if variant == 'no avg_normals':
            assert an.untouched()
        else:
            assert_close(torch.tensor(an.get().reshape(nnum, 3)), torch.tensor(rn), np.abs(rn), T.POINTS_C_NORMAL, 'avg_normals')
        if nnum == BIG:
            break                                                  # the NULL arguments take no other path at this size


def test_features_without_points():
    """n_pts = 0: zero rows everywhere; the point arrays may be NULL"""
    nk = _up(np.arange(9), torch.int64)
    feat, ap, an = Guarded(36, torch.float32), Guarded(27, torch.float32), Guarded(27, torch.float32)
    _call('ofx_octree_point_features', None, None, 0, None, 3, None, 3, _p(nk), 9, DEPTH, feat.ptr, ap.ptr, an.ptr)
    assert np.all(_bits(feat.get()) == 0) and np.all(_bits(ap.get()) == 0) and np.all(_bits(an.get()) == 0)


def test_features_refusals():
    node_keys, pts, nrm, sk, si = _feature_case(7, 1)
    n = len(pts)
    pw, nw = Window(n, 3, 3, 0, pts), Window(n, 3, 3, 0, nrm)
    skd, sid, nkd = _up(sk, torch.int64), _up(si, torch.int32), _up(node_keys, torch.int64)
    feat, ap, an = Guarded(32, torch.float32), Guarded(21, torch.float32), Guarded(21, torch.float32)
    ok = dict(sk=_p(skd), si=_p(sid), n=n, pts=pw.ptr, ldp=3, nrm=nw.ptr, ldn=3, nk=_p(nkd), nnum=7, depth=DEPTH,
              feat=feat.ptr)
    for bad in (dict(n=-1), dict(nnum=-1), dict(depth=0), dict(depth=17), dict(ldp=2), dict(ldn=2), dict(nk=None),
                dict(sk=None), dict(si=None), dict(pts=None), dict(feat=feat.ptr + 4)):
        a = dict(ok, **bad)
        _refused('ofx_octree_point_features', a['sk'], a['si'], a['n'], a['pts'], a['ldp'], a['nrm'], a['ldn'], a['nk'],
                 a['nnum'], a['depth'], a['feat'], ap.ptr, an.ptr)
    _settled(feat, ap, an)
