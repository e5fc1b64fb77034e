"""The scan and the octree container kernels (csrc/ofx_octree.hip) one entry point at a time through the C ABI, against
tests/octree_oracle.py -- bit for bit.  Every output, and the scan workspace (sized exactly ofx_scan_ws_bytes(n)), sits
between sentinel bands that must come back untouched.

    entry point               cases                                                              refusals (OFX_EINVAL)
    ofx_scan_i32              test_scan (n = 0, 1, tile edges 2047..2049, 256 / 257 tiles,       n < 0, NULL out / ws / in
                              a total of exactly 2^31 - 1)
    ofx_octree_full_layer     test_full_layer (depth 0..4, B 1 / 3)                              depth < 0, > 10, B < 1, NULLs
    ofx_octree_split          test_split (labels 0, 1, 2, -1, INT32_MIN; n = 0, 1, 2049)         n < 0, NULL label / children /
                                                                                                 scan_out / ws
    ofx_octree_grow           test_grow (absent children, batch ids > 0, depth-8 keys,           n < 0, NULL outputs, NULL inputs
                              n_parent = 0)                                                      with n > 0
    ofx_split_small_label0/1  test_split_small (full_depth 0..3, B 1 / 3, special values)        NULLs, B < 1, full_depth < 0, > 8
    ofx_split_large_label0/1  test_split_large (n = 0, 1, 257, special values)                   n < 0, NULLs with n > 0, a split
                                                                                                 4 bytes off 16 (label0)
    ofx_octree2voxel_cf,      test_voxel_layouts (depth 0..3, B 1 / 3 / 9, C 1 / 63 / 64 / 65 /  NULLs, C < 1, B < 1, depth < 0,
    ofx_voxel2octree_cf       130, rows contiguous and as a column window ld = C + 3)            > 8, ld < C

The special values of the `> 0` threshold: 0.0, -0.0, the smallest denormal of either sign, the infinities and NaN.
"""
import numpy as np
import pytest
import torch

import octree_oracle as O
from test_gpu_fullwidth import dev
from test_gpu_graph_tables import SENT, Guarded, _p, _up

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

INT32_MIN = -2 ** 31


def _call(name, *args):
    from octfusion_amd._lib import call, stream
    return call(name, *args, stream())


def _refused(name, *args):
    from octfusion_amd import _lib
    with pytest.raises(_lib.OfxError, match='invalid argument'):
        _call(name, *args)


def _ws(n):
    from octfusion_amd import _lib
    nbytes = int(_lib.lib().ofx_scan_ws_bytes(n))
    assert nbytes % 4 == 0 and nbytes >= 8
    return Guarded(nbytes // 4, torch.int32)


def _settled(*guards):
    torch.cuda.synchronize()
    for g in guards:
        assert g.untouched()


# ------------------------------------------------------------------------------------------------ scan
def _scan_values(n, seed):
    return np.random.default_rng(seed).integers(0, 5, size=n)


@pytest.mark.parametrize('n', [0, 1, 2047, 2048, 2049, 524287, 524288, 524289, 'total'])
def test_scan(n):
    if n == 'total':                                               # 2048 (2^20 - 1) + 2047 = 2^31 - 1, over two tiles
        v = np.full(2049, 2 ** 20 - 1, dtype=np.int64)
        v[-1] = 2047
        assert int(v.sum()) == 2 ** 31 - 1
    else:
        v = _scan_values(n, n)
    src = _up(v, torch.int32)
    out, ws = Guarded(len(v) + 1, torch.int32), _ws(len(v))
    _call('ofx_scan_i32', _p(src), out.ptr, len(v), ws.ptr)
    assert np.array_equal(out.get(), O.exclusive_scan(v))
    assert ws.bands_intact()
    if len(v) == 0:
        assert out.get()[0] == 0
        out2 = Guarded(1, torch.int32)
        _call('ofx_scan_i32', None, out2.ptr, 0, ws.ptr)           # nothing to read: a NULL input is accepted
        assert out2.get()[0] == 0


def test_scan_refusals():
    src = _up(_scan_values(100, 0), torch.int32)
    out, ws = Guarded(101, torch.int32), _ws(100)
    _refused('ofx_scan_i32', _p(src), out.ptr, -1, ws.ptr)
    _refused('ofx_scan_i32', _p(src), None, 100, ws.ptr)
    _refused('ofx_scan_i32', _p(src), out.ptr, 100, None)
    _refused('ofx_scan_i32', None, out.ptr, 100, ws.ptr)
    _settled(out, ws)


# ------------------------------------------------------------------------------------------------ full layer, split, grow
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('depth', range(5))
def test_full_layer(depth, B):
    n = B * 8 ** depth
    keys, children = Guarded(n, torch.int64), Guarded(n, torch.int32)
    _call('ofx_octree_full_layer', depth, B, keys.ptr, children.ptr)
    wk, wc = O.full_layer(depth, B)
    assert np.array_equal(keys.get(), wk) and np.array_equal(children.get(), wc)
    assert np.array_equal(children.get(), np.arange(n)) and np.array_equal(keys.get() >> 48, np.arange(n) // 8 ** depth)


def test_full_layer_refusals():
    keys, children = Guarded(8, torch.int64), Guarded(8, torch.int32)
    for depth, B, k, c in ((-1, 1, keys.ptr, children.ptr), (11, 1, keys.ptr, children.ptr), (1, 0, keys.ptr, children.ptr),
                           (1, -2, keys.ptr, children.ptr), (1, 1, None, children.ptr), (1, 1, keys.ptr, None)):
        _refused('ofx_octree_full_layer', depth, B, k, c)
    _settled(keys, children)


@pytest.mark.parametrize('n', [0, 1, 2049])
def test_split(n):
    g = np.random.default_rng(n)
    label = np.array([0, 1, 2, -1, INT32_MIN], dtype=np.int64)[g.integers(0, 5, size=n)]
    if n == 1:
        label[0] = INT32_MIN
    src = _up(label, torch.int32)
    children, scan, ws = Guarded(n, torch.int32), Guarded(n + 1, torch.int32), _ws(n)
    _call('ofx_octree_split', _p(src), n, children.ptr, scan.ptr, ws.ptr)
    wc, wscan = O.split(label)
    assert np.array_equal(children.get(), wc) and np.array_equal(scan.get(), wscan)
    assert scan.get()[n] == int((label != 0).sum()) and np.all(children.get()[label == 0] == -1)
    assert ws.bands_intact()


def test_split_refusals():
    src = _up(np.ones(10), torch.int32)
    children, scan, ws = Guarded(10, torch.int32), Guarded(11, torch.int32), _ws(10)
    _refused('ofx_octree_split', _p(src), -1, children.ptr, scan.ptr, ws.ptr)
    _refused('ofx_octree_split', None, 10, children.ptr, scan.ptr, ws.ptr)
    _refused('ofx_octree_split', _p(src), 10, None, scan.ptr, ws.ptr)
    _refused('ofx_octree_split', _p(src), 10, children.ptr, None, ws.ptr)
    _refused('ofx_octree_split', _p(src), 10, children.ptr, scan.ptr, None)
    _settled(children, scan, ws)


@pytest.mark.parametrize('depth,n_parent', [(2, 0), (2, 1), (3, 37), (8, 700)])
def test_grow(depth, n_parent):
    """parents of `depth` anywhere in elements 0..4; about half have no children; their slots keep the sentinel"""
    g = np.random.default_rng(depth * 100 + n_parent)
    keys = np.sort(g.choice(8 ** min(depth, 6), size=n_parent, replace=False)).astype(np.int64) << (3 * (depth - min(depth, 6)))
    keys |= g.integers(0, 8 ** (depth - min(depth, 6)), size=n_parent)          # the low levels of a deep key
    keys |= np.sort(g.integers(0, 5, size=n_parent)).astype(np.int64) << 48
    label = g.integers(0, 2, size=n_parent)
    if n_parent == 1:
        label[0], keys[0] = 1, (8 ** depth - 1) | (4 << 48)
    children, scan = O.split(label)
    n_child = 8 * int(scan[-1]) + 8                                # one octet more than any parent points at
    kp, cp = _up(keys, torch.int64), _up(children, torch.int32)
    kc, cc = Guarded(n_child, torch.int64), Guarded(n_child, torch.int32)
    _call('ofx_octree_grow', _p(kp), _p(cp), n_parent, kc.ptr, cc.ptr)
    wk, wc = O.grow(keys, children, np.full(n_child, SENT[torch.int64], dtype=np.int64),
                    np.full(n_child, SENT[torch.int32], dtype=np.int64))
    assert np.array_equal(kc.get(), wk) and np.array_equal(cc.get(), wc)
    assert np.all(kc.get()[-8:] == SENT[torch.int64])
    if n_parent == 0:
        _call('ofx_octree_grow', None, None, 0, kc.ptr, cc.ptr)    # nothing to read
        _settled(kc, cc)


def test_grow_refusals():
    kp, cp = _up(np.arange(4), torch.int64), _up(np.arange(4), torch.int32)
    kc, cc = Guarded(32, torch.int64), Guarded(32, torch.int32)
    _refused('ofx_octree_grow', _p(kp), _p(cp), -1, kc.ptr, cc.ptr)
    _refused('ofx_octree_grow', _p(kp), _p(cp), 4, None, cc.ptr)
    _refused('ofx_octree_grow', _p(kp), _p(cp), 4, kc.ptr, None)
    _refused('ofx_octree_grow', _p(kp), _p(cp), 0, None, cc.ptr)
    _refused('ofx_octree_grow', None, _p(cp), 4, kc.ptr, cc.ptr)
    _refused('ofx_octree_grow', _p(kp), None, 4, kc.ptr, cc.ptr)
    _settled(kc, cc)


# ------------------------------------------------------------------------------------------------ split -> labels
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('fd', range(4))
def test_split_small(fd, B):
    S = 1 << fd
    sp = O.special_split((B, 8, S, S, S), 10 * fd + B)
    src = torch.tensor(sp).to(dev())
    n = B * 8 ** fd
    label = Guarded(n, torch.int32)
    _call('ofx_split_small_label0', src.data_ptr(), B, fd, label.ptr)
    want0 = O.split_small_label0(sp, fd)
    assert np.array_equal(label.get(), want0)
    children, scan = O.split(want0)
    children[::3] = -1                                             # absent children beyond those of label0: rows untouched
    cd = _up(children, torch.int32)
    label1 = Guarded(8 * int(scan[-1]) + 8, torch.int32)
    _call('ofx_split_small_label1', src.data_ptr(), B, fd, _p(cd), label1.ptr)
    want1 = O.split_small_label1(sp, fd, children, np.full(label1.n, SENT[torch.int32], dtype=np.int64))
    assert np.array_equal(label1.get(), want1)
    assert np.all(label1.get()[-8:] == SENT[torch.int32])
    got = label1.get()
    assert set(got[got != SENT[torch.int32]].tolist()) <= {0, 1}


def test_split_small_refusals():
    src = torch.zeros(1, 8, 2, 2, 2, device=dev())
    cd = _up(np.arange(8), torch.int32)
    label, label1 = Guarded(8, torch.int32), Guarded(64, torch.int32)
    for s, B, fd, out in ((None, 1, 1, label.ptr), (src.data_ptr(), 1, 1, None), (src.data_ptr(), 0, 1, label.ptr),
                          (src.data_ptr(), 1, -1, label.ptr), (src.data_ptr(), 1, 9, label.ptr)):
        _refused('ofx_split_small_label0', s, B, fd, out)
    for s, B, fd, c, out in ((None, 1, 1, _p(cd), label1.ptr), (src.data_ptr(), 1, 1, None, label1.ptr),
                             (src.data_ptr(), 1, 1, _p(cd), None), (src.data_ptr(), 0, 1, _p(cd), label1.ptr),
                             (src.data_ptr(), 1, -1, _p(cd), label1.ptr), (src.data_ptr(), 1, 9, _p(cd), label1.ptr)):
        _refused('ofx_split_small_label1', s, B, fd, c, out)
    _settled(label, label1)


@pytest.mark.parametrize('n', [0, 1, 257])
def test_split_large(n):
    sp = O.special_split((n, 8), 77 + n)
    if n == 1:
        sp[0] = [0.0, -0.0, -1e-45, -np.inf, np.nan, -1.0, 1e-45, -2.0]      # the smallest denormal alone decides
    src = _up(sp, torch.float32)
    assert _p(src) % 16 == 0
    label0 = Guarded(n, torch.int32)
    _call('ofx_split_large_label0', _p(src), n, label0.ptr)
    want0 = O.split_large_label0(sp)
    assert np.array_equal(label0.get(), want0)
    if n == 1:
        assert want0[0] == 1
    children, scan = O.split(want0)
    children[::3] = -1
    cd = _up(children, torch.int32)
    label1 = Guarded(8 * int(scan[-1]) + 8, torch.int32)
    _call('ofx_split_large_label1', _p(src), n, _p(cd), label1.ptr)
    want1 = O.split_large_label1(sp, children, np.full(label1.n, SENT[torch.int32], dtype=np.int64))
    assert np.array_equal(label1.get(), want1)
    if n == 0:
        _call('ofx_split_large_label0', None, 0, None)
        _call('ofx_split_large_label1', None, 0, None, None)
        _settled(label0, label1)


def test_split_large_refusals():
    buf = torch.zeros(8 * 8 + 4, device=dev())
    assert buf.data_ptr() % 16 == 0
    cd = _up(np.arange(8), torch.int32)
    label0, label1 = Guarded(8, torch.int32), Guarded(64, torch.int32)
    _refused('ofx_split_large_label0', buf.data_ptr() + 4, 8, label0.ptr)          # 4 bytes off a 16-byte boundary
    _refused('ofx_split_large_label0', buf.data_ptr(), -1, label0.ptr)
    _refused('ofx_split_large_label0', None, 8, label0.ptr)
    _refused('ofx_split_large_label0', buf.data_ptr(), 8, None)
    _refused('ofx_split_large_label1', buf.data_ptr(), -1, _p(cd), label1.ptr)
    _refused('ofx_split_large_label1', None, 8, _p(cd), label1.ptr)
    _refused('ofx_split_large_label1', buf.data_ptr(), 8, None, label1.ptr)
    _refused('ofx_split_large_label1', buf.data_ptr(), 8, _p(cd), None)
    _settled(label0, label1)


# ------------------------------------------------------------------------------------------------ rows <-> voxels
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize('B', [1, 3, 9])
@pytest.mark.parametrize('depth', range(4))
def test_voxel_layouts(depth, B):
    rows, S = B * 8 ** depth, 1 << depth
    sent = np.float32(SENT[torch.float32])
    for C in (1, 63, 64, 65, 130):
        data = np.random.default_rng(1000 * depth + 10 * B + C).standard_normal((rows, C)).astype(np.float32)
        want_vox = O.octree2voxel_cf(data, B, depth)
        assert np.array_equal(O.voxel2octree_cf(want_vox, depth), data)
        for ld, col0 in ((C, 0), (C + 3, 2)):
            # rows -> voxels: the rows sit in a sentinel-filled [rows, ld] buffer at column col0
            src = Guarded(rows * ld, torch.float32)
            src.view.view(rows, ld)[:, col0:col0 + C] = torch.tensor(data).to(dev())
            vox = Guarded(B * C * S ** 3, torch.float32)
            _call('ofx_octree2voxel_cf', src.ptr + 4 * col0, ld, C, B, depth, vox.ptr)
            assert np.array_equal(_bits(vox.get()), _bits(want_vox).reshape(-1)), (C, ld)
            # voxels -> rows, into the window of a sentinel-filled buffer; then the round trip
            for source in (torch.tensor(want_vox).to(dev()).reshape(-1), vox.view):
                dst = Guarded(rows * ld, torch.float32)
                _call('ofx_voxel2octree_cf', source.data_ptr(), C, B, depth, dst.ptr + 4 * col0, ld)
                got = dst.get().reshape(rows, ld)
                assert np.array_equal(_bits(got[:, col0:col0 + C]), _bits(data)), (C, ld)
                rest = np.delete(got, np.s_[col0:col0 + C], axis=1)
                assert np.all(_bits(rest) == _bits(sent)), (C, ld)
            assert vox.bands_intact() and src.bands_intact()


def test_voxel_refusals():
    data, vox = Guarded(64 * 4, torch.float32), Guarded(64 * 4, torch.float32)
    ok = dict(data=data.ptr, ld=4, C=4, B=1, depth=2, vox=vox.ptr)
    for bad in (dict(data=None), dict(vox=None), dict(C=0), dict(B=0), dict(depth=-1), dict(depth=9), dict(ld=3)):
        a = dict(ok, **bad)
        _refused('ofx_octree2voxel_cf', a['data'], a['ld'], a['C'], a['B'], a['depth'], a['vox'])
        _refused('ofx_voxel2octree_cf', a['vox'], a['C'], a['B'], a['depth'], a['data'], a['ld'])
    _settled(data, vox)
