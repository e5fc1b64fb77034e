"""The NeuralMPU entry points (second half of csrc/ofx_graph.hip) one at a time through the C ABI, against the float64
restatement tests/mpu_oracle.py, on the deep ragged trees of tests/graph_oracle.py put on the device from the ORACLE
octree's arrays (nothing of octree.py takes part).  Every output window lies between sentinel bands that must survive.

Bounds (mpu_oracle.bounds; no point is excluded from any comparison):
    |sdf  - ref| <= gamma(K_sdf)  S / D         S = sum w_i (|c_i0 f s| + |c_i1 f s| + |c_i2 f s| + |c_i3|)
    |grad - ref| <= gamma(K_grad) * (sum of absolute values of every term of dn / D - num dd / D^2)
    |dcode - ref| <= gamma(K_dcode + m_row) * (sum of absolute values of the element's contributions and of its start)
with gamma(k) = k 2^-24 / (1 - k 2^-24) and, for nd = depth_end - depth_start + 1 depths, the constants counted from the
kernels' chains of float32 operations (the counts are spelled out in mpu_oracle.k_sdf / k_grad / k_dcode):
    K_sdf   = 26 + 2 nd   num: 4 (v) + 6 (w) + 1 (w v) + nd (depths) + 3 (shuffles); D: 6 + nd + 3 + 1 (+ eps); 2 (1 / D, *)
    K_grad  = 48 + 4 nd   dn / D: 26 + 2 nd; (num / D / D) dd: 47 + 4 nd; the subtraction: 1
    K_dcode = 46 + 3 nd   A_i: 44 + 3 nd; A f s + b w / D: 2; the m_row atomic additions come on top, in any order
The constants come from the code, not from what the GPU produced.  Worst |got - ref| / bound, printed by the last test:
    measured on an MI355X                  sdf 0.162 (ofx_mpu_eval), 0.162 (ofx_mpu_eval_grad)   grad 0.066   dcode 0.103
    oracle/mpu.py, float32, on the host    sdf 0.196                                             grad 0.062   dcode 0.106
(the second line over the 4099-point inputs of every tree and depth range, grad and dcode by float32 autograd:
tests/test_mpu_oracle.py prints it).

Outside the contract, and in no case here: NaN or infinite coordinates or batch ids (the reference's .short() is undefined
there), and the 2^31 limits on the point count (they would need gigabytes).

    entry point         cases                                                         refusals (OFX_EINVAL, outputs unchanged)
    ofx_mpu_eval        test_points (4 trees x 5 depth ranges x 1, 7, 8, 33, 4099     pts NULL / 4 bytes off 16; code NULL / off;
                        points; mask and mask = NULL), test_grid (the explicit        sdf NULL; de > depth, ds < 0, de < ds, n < 0, > 2^31;
                        lattice), test_nothing_to_see                                 every make_tree check; n = 0 is OK
    ofx_mpu_eval_grid   test_grid (sizes 5, 33; four windows; batch indices 0, 1)     size < 1, head < 0, count < 0, head + count >
                                                                                      size^3, and the shared checks above
    ofx_mpu_eval_grad   test_points, test_nothing_to_see                              as eval, + grad NULL
    ofx_mpu_backward    test_points (both upstreams, each alone, into a random        as eval, + dcode NULL, both upstreams NULL
                        table, twice), test_nothing_to_see
"""
import ctypes

import numpy as np
import pytest
import torch

import mpu_oracle as M
from test_gpu_fullwidth import dev, report
from test_gpu_graph_tables import Guarded, _dev_tree
from test_mpu_oracle import RANGE_IDS, TREES, case, key_tree

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

WORST = {'sdf_eval': 0.0, 'sdf_eval_grad': 0.0, 'grad': 0.0, 'dcode': 0.0}


def _call(name, *args):
    from octfusion_amd._lib import call, stream
    return call(name, *args, stream())


def _refused(name, *args):
    from octfusion_amd import _lib
    with pytest.raises(_lib.OfxError, match='invalid argument'):
        _call(name, *args)


def _dev(a, dtype=torch.float32):
    """host array -> device tensor with at least one element behind it (16-byte aligned)"""
    t = torch.as_tensor(np.ascontiguousarray(a)).to(dtype).reshape(-1)
    t = torch.cat([t, torch.zeros(4, dtype=dtype)]).to(dev())
    assert t.data_ptr() % 16 == 0
    return t


def _ratio(what, got, ref, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(err == 0, 0.0, err / bound)
    r = float(q.max()) if q.size else 0.0
    WORST[what] = max(WORST[what], r)
    return r


def _eval(T, ds, de, pts_d, n, code_d, with_mask=True):
    sdf, mask = Guarded(n, torch.float32), Guarded(n, torch.uint8)
    _call('ofx_mpu_eval', ctypes.byref(T.tree), ds, de, pts_d.data_ptr(), n, code_d.data_ptr(), sdf.ptr,
          mask.ptr if with_mask else None)
    if not with_mask:
        assert mask.untouched()
    return sdf, mask


def _eval_grad(T, ds, de, pts_d, n, code_d, with_mask=True):
    sdf, grad, mask = Guarded(n, torch.float32), Guarded(3 * n, torch.float32), Guarded(n, torch.uint8)
    _call('ofx_mpu_eval_grad', ctypes.byref(T.tree), ds, de, pts_d.data_ptr(), n, code_d.data_ptr(), sdf.ptr, grad.ptr,
          mask.ptr if with_mask else None)
    if not with_mask:
        assert mask.untouched()
    return sdf, grad, mask


def _backward(T, ds, de, pts_d, n, code_d, dsdf_d, dgrad_d, start):
    """dcode after one ofx_mpu_backward into a table that starts as `start` (host [rows, 4]); the Guarded itself"""
    dcode = Guarded(start.size, torch.float32)
    dcode.view.copy_(torch.as_tensor(start.reshape(-1)).to(dev()))
    _call('ofx_mpu_backward', ctypes.byref(T.tree), ds, de, pts_d.data_ptr(), n, code_d.data_ptr(),
          None if dsdf_d is None else dsdf_d.data_ptr(), None if dgrad_d is None else dgrad_d.data_ptr(), dcode.ptr)
    return dcode


# ------------------------------------------------------------------------------------------------ explicit points
@pytest.mark.parametrize('ri', range(5), ids=RANGE_IDS)
@pytest.mark.parametrize('name', TREES)
def test_points(name, ri):
    T = _dev_tree(name)
    for n in M.COUNTS:
        K, ds, de, pts, kind, code, dsdf, dgrad, R = case(name, ri, n)
        nd = de - ds + 1
        b_sdf, b_grad, b_dcode = M.bounds(R, nd)
        pts_d, code_d, dsdf_d, dgrad_d = _dev(pts), _dev(code), _dev(dsdf), _dev(dgrad)
        nothing = R['used'] == 0                                   # no centre contributes: exact zeros
        bid = M.batch_of(pts)
        assert np.all(nothing[(bid < 0) | (bid >= K.batch_size)])
        if ds > K.full_depth:
            assert np.all(nothing[kind == 7])                      # an empty element has nothing below its full layer
        # ofx_mpu_eval
        sdf, mask = _eval(T, ds, de, pts_d, n, code_d)
        assert np.array_equal(mask.get(), R['mask'].astype(np.int64)), 'mask'
        r = _ratio('sdf_eval', sdf.get(), R['sdf'], b_sdf)
        assert r <= 1.0, ('sdf', n, r)
        assert np.all(sdf.get()[nothing] == 0) and np.all(mask.get()[nothing & ~R['mask']] == 0)
        sdf2, _ = _eval(T, ds, de, pts_d, n, code_d, with_mask=False)
        assert torch.equal(sdf.buf, sdf2.buf)
        # ofx_mpu_eval_grad
        gsdf, grad, gmask = _eval_grad(T, ds, de, pts_d, n, code_d)
        assert np.array_equal(gmask.get(), R['mask'].astype(np.int64)), 'mask of eval_grad'
        r = _ratio('sdf_eval_grad', gsdf.get(), R['sdf'], b_sdf)
        assert r <= 1.0, ('sdf of eval_grad', n, r)
        r = _ratio('grad', grad.get().reshape(n, 3), R['grad'], b_grad)
        assert r <= 1.0, ('grad', n, r)
        assert np.all(gsdf.get()[nothing] == 0) and np.all(grad.get().reshape(n, 3)[nothing] == 0)
        gsdf2, grad2, _ = _eval_grad(T, ds, de, pts_d, n, code_d, with_mask=False)
        assert torch.equal(gsdf.buf, gsdf2.buf) and torch.equal(grad.buf, grad2.buf)
        # ofx_mpu_backward: both upstreams into zeros, twice
        zero = np.zeros_like(code)
        runs = [_backward(T, ds, de, pts_d, n, code_d, dsdf_d, dgrad_d, zero).get().reshape(-1, 4) for _ in range(2)]
        for got in runs:
            r = _ratio('dcode', got, R['dcode'], b_dcode)
            assert r <= 1.0, ('dcode', n, r)
        # two runs differ by the order of the m_row additions alone
        assert np.all(np.abs(runs[0].astype(np.float64) - runs[1]) <= 2 * M.gamma(R['m_row'])[:, None] * R['dabs'])
        assert np.all(runs[0][R['m_row'] == 0] == 0)
        # each upstream alone; their sum is the joint result
        Ra = M.evaluate(K, ds, de, pts, code, dsdf, None)
        Rb = M.evaluate(K, ds, de, pts, code, None, dgrad)
        ga = _backward(T, ds, de, pts_d, n, code_d, dsdf_d, None, zero).get().reshape(-1, 4)
        gb = _backward(T, ds, de, pts_d, n, code_d, None, dgrad_d, zero).get().reshape(-1, 4)
        ba, bb = M.bounds(Ra, nd)[2], M.bounds(Rb, nd)[2]
        assert _ratio('dcode', ga, Ra['dcode'], ba) <= 1.0 and _ratio('dcode', gb, Rb['dcode'], bb) <= 1.0
        assert _ratio('dcode', ga.astype(np.float64) + gb, R['dcode'], ba + bb) <= 1.0
        # accumulation into a table that is not zero
        start = np.random.default_rng(n).standard_normal(code.shape).astype(np.float32)
        Rs = M.evaluate(K, ds, de, pts, code, dsdf, dgrad, dcode0=start)
        gs = _backward(T, ds, de, pts_d, n, code_d, dsdf_d, dgrad_d, start).get().reshape(-1, 4)
        r = _ratio('dcode', gs, Rs['dcode'], M.bounds(Rs, nd)[2])
        assert r <= 1.0, ('dcode into a random table', n, r)
        assert np.array_equal(gs[Rs['m_row'] == 0].view(np.int32), start[Rs['m_row'] == 0].view(np.int32))


# ------------------------------------------------------------------------------------------------ the lattice sweep
@pytest.mark.parametrize('size', [5, 33])
@pytest.mark.parametrize('name', ['deep_a', 'deep_b_mid'])
def test_grid(name, size):
    T, K = _dev_tree(name), key_tree(name)
    ds, de = M.ranges(K)[0]
    code = M.code_table(K, ds, de, seed=3)
    code_d = _dev(code)
    bbmin, bbmax = -0.9, 0.9
    step = (bbmax - bbmin) / size
    total = size ** 3
    mid = total // 3
    windows = [(0, total), (mid, (total // 2) | 1), (total - 1, 1), (mid, 0), (total, 0)]
    assert windows[1][1] % 2 == 1 and mid + windows[1][1] < total
    for batch in (0, 1):
        for head, count in windows:
            sdf, mask = Guarded(count, torch.float32), Guarded(count, torch.uint8)
            _call('ofx_mpu_eval_grid', ctypes.byref(T.tree), ds, de, code_d.data_ptr(), size, step, bbmin, batch, head, count,
                  sdf.ptr, mask.ptr)
            if count == 0:
                torch.cuda.synchronize()
                assert sdf.untouched() and mask.untouched()
                continue
            pts = M.lattice(size, step, bbmin, batch, head, count)
            assert pts.shape == (count, 4)
            esdf, emask = _eval(T, ds, de, _dev(pts), count, code_d)
            assert torch.equal(sdf.buf, esdf.buf) and torch.equal(mask.buf, emask.buf), (batch, head, count)
            R = M.evaluate(K, ds, de, pts, code)
            assert np.array_equal(mask.get(), R['mask'].astype(np.int64))
            assert _ratio('sdf_eval', sdf.get(), R['sdf'], M.bounds(R, de - ds + 1)[0]) <= 1.0
            sdf2 = Guarded(count, torch.float32)
            _call('ofx_mpu_eval_grid', ctypes.byref(T.tree), ds, de, code_d.data_ptr(), size, step, bbmin, batch, head, count,
                  sdf2.ptr, None)
            assert torch.equal(sdf.buf, sdf2.buf)


# ------------------------------------------------------------------------------------------------ nothing but misses
@pytest.mark.parametrize('name', ['deep_a', 'deep_b_mid'])
def test_nothing_to_see(name):
    """a batch made only of points in an empty element and of out-of-range batch ids: zeros out, dcode bit-unchanged"""
    T, K = _dev_tree(name), key_tree(name)
    ds, de = M.ranges(K)[2]                                        # below the full layer an empty element has no node
    B = K.batch_size
    pts, _ = M.points(K, ds, de, 37, seed=9)
    ids = [-1.0, float(B), float(B + 3), -7.5, B + 0.25] + [float(b) for b in M.empty_elements(K)]
    pts[:, 3] = np.array(ids, dtype=np.float32)[np.arange(37) % len(ids)]
    code = M.code_table(K, ds, de, seed=4)
    R = M.evaluate(K, ds, de, pts, code)
    assert np.all(R['used'] == 0) and not R['mask'].any()
    pts_d, code_d = _dev(pts), _dev(code)
    sdf, mask = _eval(T, ds, de, pts_d, 37, code_d)
    gsdf, grad, gmask = _eval_grad(T, ds, de, pts_d, 37, code_d)
    for o in (sdf, mask, gsdf, grad, gmask):
        assert np.all(o.get() == 0)
    start = np.random.default_rng(1).standard_normal(code.shape).astype(np.float32)
    up = np.random.default_rng(2).standard_normal((37, 4)).astype(np.float32)
    got = _backward(T, ds, de, pts_d, 37, code_d, _dev(up[:, 0]), _dev(up[:, 1:]), start).get()
    assert np.array_equal(got.view(np.int32), start.reshape(-1).view(np.int32))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from octfusion_amd import _lib
    T, K = _dev_tree('deep_a'), key_tree('deep_a')
    ds, de = M.ranges(K)[0]
    n = 33
    pts, _ = M.points(K, ds, de, n)
    code = M.code_table(K, ds, de)
    pts_d, code_d = _dev(pts), _dev(code)
    up_d = _dev(np.ones(4 * n, dtype=np.float32))
    sdf, grad, mask = Guarded(n, torch.float32), Guarded(3 * n, torch.float32), Guarded(n, torch.uint8)
    dcode = Guarded(code.size, torch.float32)
    tree = ctypes.byref(T.tree)
    P, C, U = pts_d.data_ptr(), code_d.data_ptr(), up_d.data_ptr()

    def all_four(tree=tree, ds=ds, de=de, P=P, n=n, C=C, only=None):
        """the same bad argument through every entry point that takes it"""
        if only in (None, 'eval'):
            _refused('ofx_mpu_eval', tree, ds, de, P, n, C, sdf.ptr, mask.ptr)
        if only in (None, 'grad'):
            _refused('ofx_mpu_eval_grad', tree, ds, de, P, n, C, sdf.ptr, grad.ptr, mask.ptr)
        if only in (None, 'backward'):
            _refused('ofx_mpu_backward', tree, ds, de, P, n, C, U, U, dcode.ptr)
        if only in (None, 'grid') and P == pts_d.data_ptr() and n == 33:
            _refused('ofx_mpu_eval_grid', tree, ds, de, C, 4, 0.5, -1.0, 0, 0, n, sdf.ptr, mask.ptr)

    all_four(C=C + 4)                                              # code 4 bytes off a 16-byte boundary
    all_four(C=None)
    all_four(P=P + 4)
    all_four(P=None)
    all_four(de=K.depth + 1)
    all_four(ds=-1)
    all_four(ds=de, de=ds)
    all_four(n=-1)
    _refused('ofx_mpu_eval_grid', tree, ds, de, C, 4, 0.5, -1.0, 0, 0, -1, sdf.ptr, mask.ptr)
    all_four(n=2 ** 31 + 1)                                        # refused by the count alone: nothing is read
    _refused('ofx_mpu_eval_grid', tree, ds, de, C, 1300, 0.001, -1.0, 0, 0, 2 ** 31 + 1, sdf.ptr, mask.ptr)
    # NULL outputs, both upstreams NULL
    _refused('ofx_mpu_eval', tree, ds, de, P, n, C, None, mask.ptr)
    _refused('ofx_mpu_eval_grid', tree, ds, de, C, 4, 0.5, -1.0, 0, 0, n, None, mask.ptr)
    _refused('ofx_mpu_eval_grad', tree, ds, de, P, n, C, None, grad.ptr, mask.ptr)
    _refused('ofx_mpu_eval_grad', tree, ds, de, P, n, C, sdf.ptr, None, mask.ptr)
    _refused('ofx_mpu_backward', tree, ds, de, P, n, C, U, U, None)
    _refused('ofx_mpu_backward', tree, ds, de, P, n, C, None, None, dcode.ptr)
    # the lattice window
    for size, head, count in ((0, 0, 0), (-3, 0, 1), (4, -1, 2), (4, 60, 5), (4, 64, 1), (4, 0, 65)):
        _refused('ofx_mpu_eval_grid', tree, ds, de, C, size, 0.5, -1.0, 0, head, count, sdf.ptr, mask.ptr)
    # make_tree
    oc = T.oc
    nn, ne = ctypes.addressof(T._nnum_c), ctypes.addressof(T._nne_c)
    ch, ke, rk = T.child.data_ptr(), T.key.data_ptr(), T.rank.ptr
    bad_trees = [_lib.OfxTree(oc.depth, oc.depth + 1, oc.batch_size, ch, ke, rk, nn, ne),     # full_depth > depth
                 _lib.OfxTree(oc.depth, -1, oc.batch_size, ch, ke, rk, nn, ne),
                 _lib.OfxTree(-1, -1, oc.batch_size, ch, ke, rk, nn, ne),
                 _lib.OfxTree(17, oc.full_depth, oc.batch_size, ch, ke, rk, nn, ne),
                 _lib.OfxTree(oc.depth, oc.full_depth, 0, ch, ke, rk, nn, ne),
                 _lib.OfxTree(oc.depth, oc.full_depth, oc.batch_size, None, ke, rk, nn, ne),
                 _lib.OfxTree(oc.depth, oc.full_depth, oc.batch_size, ch, None, rk, nn, ne),
                 _lib.OfxTree(oc.depth, oc.full_depth, oc.batch_size, ch, ke, rk, None, ne),
                 _lib.OfxTree(oc.depth, oc.full_depth, oc.batch_size, ch, ke, rk, nn, None)]
    for bt in bad_trees:
        all_four(tree=ctypes.byref(bt), de=min(de, 6))
    all_four(tree=None)
    torch.cuda.synchronize()
    for o in (sdf, grad, mask, dcode):
        assert o.untouched()
    # n == 0 is no error and touches nothing; a tree without leaf ranks is fine (the MPU does not read them)
    _call('ofx_mpu_eval', tree, ds, de, P, 0, C, sdf.ptr, mask.ptr)
    _call('ofx_mpu_eval_grad', tree, ds, de, P, 0, C, sdf.ptr, grad.ptr, mask.ptr)
    _call('ofx_mpu_backward', tree, ds, de, P, 0, C, U, U, dcode.ptr)
    _call('ofx_mpu_eval_grid', tree, ds, de, C, 4, 0.5, -1.0, 0, 64, 0, sdf.ptr, mask.ptr)
    torch.cuda.synchronize()
    for o in (sdf, grad, mask, dcode):
        assert o.untouched()
    no_rank = T.struct(leafrank=False)
    s2 = Guarded(n, torch.float32)
    _call('ofx_mpu_eval', ctypes.byref(no_rank), ds, de, P, n, C, s2.ptr, None)
    s3, _ = _eval(T, ds, de, pts_d, n, code_d)
    assert torch.equal(s2.buf, s3.buf)


def test_zz_worst_ratio_per_entry_point():
    """(runs last in this module) worst |got - ref| / bound over every case above, per output, measured on the GPU."""
    report({'test': 'mpu_entry_worst_ratio_to_bound', 'measured_on_gpu': True, 'worst': WORST})
    assert all(v <= 1.0 for v in WORST.values()), WORST
