"""The VAE loss kernels (csrc/ofx_loss.hip) one entry point at a time through the C ABI, against tests/train_oracle.py.
Every output sits between sentinel bands that must come back untouched; pitched operands are column windows of
sentinel-filled buffers; every case runs with its pointers on a 16-byte boundary and 4 bytes off it (the kernels load
scalars).  The fp64 accumulators are pre-filled: the contract is `sums +=`.

    entry point        cases                                                               refusals (OFX_EINVAL)
    ofx_octree_ce      test_ce: n = 0, 1, 255, 256, 257, 65 537, 2 097 152 + 257 (the      n < 0, NULL sums, NULL logits /
                       grid-stride step) of N(0, 3) rows with exact ties and +-80 rows;     child with n > 0, ld < 2,
                       test_ce_confident: +-a rows, a in 0..3, 4..8, 8..16; labels from    ldd < 2 with dlogits given
                       child in {-1, 0, INT32_MIN, INT32_MAX}; logits tight and as a
                       window ld = 5, dlogits tight and ldd = 3, dlogits NULL
    ofx_sdf_reg_loss   test_sdf_reg: the same n, w_sdf = 200, w_grad = 0.25, NULL dsdf and  n < 0, NULL sums, each NULL input
                       NULL dgrad each on its own                                          with n > 0
    ofx_kl_sample_fwd  test_kl: E = 1, 3, 4, 8 with n so that n E crosses 2 097 152; the    n < 0, E < 1, NULL params / z with
    ofx_kl_sample_bwd  log-variances -30 and 20, one ulp inside and outside each, +-40, 0;  n > 0, ld < 2E; bwd: NULL params /
                       params tight and ld = 2E + 3, dparams tight and ldp = 2E + 1; NULL   dparams, ld < 2E, ldp < 2E
                       noise (z == mean bit for bit), NULL dz, NULL kl_sum

Bounds.  The summed cross entropy: max(3 x the error of the float32 host evaluation of the oracle on the same rows,
n 2^-52 ref) (train_oracle.ce_loss_bound); the hit count exact; dlogits elementwise relative to its own value, c = 10 +
|d| (1 - s) (train_oracle.ce_grad); dlogits[:, 0] == -dlogits[:, 1] bit for bit.  sdf_reg: sums of exact non-negative
fp64 terms, n 2^-52 relative in any order (the argument of tests/test_gpu_train_kernels.py; the pre-fill is one more such
term); the gradients bit-equal to the fp32 products.  kl: glue_oracle.assert_close with the constants KL_C_* counted
next to the formulas in train_oracle; the sum of the kl terms within KL_C_TERM U sum S plus n E 2^-52 of the total.
"""
import numpy as np
import pytest
import torch

import train_oracle as T
from glue_oracle import U, assert_close
from test_gpu_fullwidth import dev
from test_gpu_graph_tables import SENT, Guarded, _p, _up

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

STRIDE = T.GRID_CAP + 257                     # the smallest of the sizes at which the grid-stride step runs
SIZES = [0, 1, 255, 256, 257, 65537, STRIDE]
FILL = (0.5, 7.0)                             # what the accumulators hold on entry (7 + hits is exact)


def _call(name, *args):
    from octfusion_amd._lib import call, stream
    return call(name, *args, stream())


def _refused(name, *args):
    from octfusion_amd import _lib
    with pytest.raises(_lib.OfxError, match='invalid argument'):
        _call(name, *args)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


class Window:
    """[rows, width] float32 at column `col0` of a sentinel-filled [rows, ld] buffer between sentinel bands; `.ptr`
    points at its first element: 4 * col0 bytes off the buffer's 16-byte boundary."""

    def __init__(self, rows, width, ld, col0=0, data=None):
        assert col0 + width <= ld
        self.rows, self.width, self.ld, self.col0 = rows, width, ld, col0
        self.g = Guarded(rows * ld, torch.float32)
        assert self.g.ptr % 16 == 0
        self.ptr = self.g.ptr + 4 * col0
        if data is not None and rows:
            self.g.view.view(rows, ld)[:, col0:col0 + width] = torch.as_tensor(np.ascontiguousarray(data)).to(dev())

    def get(self):
        """the window; everything around it must still be the sentinel"""
        a = self.g.get().reshape(self.rows, self.ld)
        rest = np.delete(a, np.s_[self.col0:self.col0 + self.width], axis=1)
        assert np.all(_bits(rest) == _bits(np.float32(SENT[torch.float32]))), 'wrote between the rows of its window'
        return a[:, self.col0:self.col0 + self.width]

    def untouched(self):
        return self.g.untouched()


def _sums(fill=FILL):
    return torch.tensor(fill, dtype=torch.float64, device=dev())


# ------------------------------------------------------------------------------------------------ ofx_octree_ce
def _ce_check(kind, n, seed, ld, lcol, ldd, dcol, dscale=0.37):
    logits, child = T.ce_case_rows(kind, n, seed)
    lw = Window(n, 2, ld, lcol, logits)
    cd = _up(child, torch.int32)
    dl = Window(n, 2, ldd, dcol)
    sums = _sums()
    _call('ofx_octree_ce', lw.ptr, ld, _p(cd), n, dscale, sums.data_ptr(), dl.ptr, ldd)
    got = sums.cpu().numpy()
    ce, _ = T.ce_rows(logits, child)
    ref = float(ce.sum())
    bound, host, host_signed = T.ce_loss_bound(logits, child, ref)
    err = abs(got[0] - FILL[0] - ref)
    print('ce %r n %d: loss %.9g ref %.9g |err| %.3e (relative %.3e) bound %.3e (ratio %.3f; host fp32: row errors %.3e, '
          'signed sum error %.3e)' % (kind, n, got[0] - FILL[0], ref, err, err / ref if ref else 0.0, bound,
                                      err / bound if bound else 0.0, host, host_signed))
    assert got[1] == FILL[1] + T.ce_hits(logits, child)
    assert err <= bound
    want, S, c = T.ce_grad(logits, child, dscale)
    g = dl.get()
    assert np.array_equal(_bits(g[:, 0]), _bits(-g[:, 1]))
    used = assert_close(torch.tensor(g), torch.tensor(want), S, torch.tensor(c), 'dlogits %r n %d' % (kind, n))
    print('ce %r n %d: dlogits uses %.3f of its bound' % (kind, n, used))
    # dlogits NULL: the same sums, the buffer untouched
    dl2, sums2 = Window(n, 2, ldd, dcol), _sums()
    _call('ofx_octree_ce', lw.ptr, ld, _p(cd), n, dscale, sums2.data_ptr(), None, ldd)
    got2 = sums2.cpu().numpy()
    assert got2[1] == got[1] and abs(got2[0] - FILL[0] - ref) <= bound
    assert dl2.untouched()
    return err / bound if bound else 0.0


@pytest.mark.parametrize('layout', ['tight', 'pitched'])
@pytest.mark.parametrize('n', SIZES)
def test_ce(n, layout):
    ld, lcol, ldd, dcol = (2, 0, 2, 0) if layout == 'tight' else (5, 1, 3, 1)
    _ce_check('mix', n, 100 + n % 1000, ld, lcol, ldd, dcol)


@pytest.mark.parametrize('n', [257, 65537])
@pytest.mark.parametrize('band', T.CE_BANDS)
def test_ce_confident(band, n):
    """correctly classified rows +-a: where m + log(e0 + e1) - l_label rounds the loss of a row to 0"""
    _ce_check(band, n, int(band[0]) + n, 5, 2, 3, 0)


def test_ce_empty_accepts_null():
    sums = _sums()
    _call('ofx_octree_ce', None, 2, None, 0, 1.0, sums.data_ptr(), None, 2)
    assert sums.cpu().tolist() == list(FILL)


def test_ce_refusals():
    logits, child = T.ce_case_rows('mix', 64, 1)
    lw, cd, dl, sums = Window(64, 2, 2, 0, logits), _up(child, torch.int32), Window(64, 2, 2), _sums()
    ok = dict(logits=lw.ptr, ld=2, child=_p(cd), n=64, sums=sums.data_ptr(), dl=dl.ptr, ldd=2)
    for bad in (dict(n=-1), dict(sums=None), dict(sums=None, n=0), dict(logits=None), dict(child=None), dict(ld=1),
                dict(ldd=1)):
        a = dict(ok, **bad)
        _refused('ofx_octree_ce', a['logits'], a['ld'], a['child'], a['n'], 1.0, a['sums'], a['dl'], a['ldd'])
    _call('ofx_octree_ce', lw.ptr, 2, _p(cd), 64, 1.0, sums.data_ptr(), None, 1)          # ldd unused without dlogits
    torch.cuda.synchronize()
    assert dl.untouched() and sums.cpu()[1] == FILL[1] + T.ce_hits(logits, child)


# ------------------------------------------------------------------------------------------------ ofx_sdf_reg_loss
@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('n', SIZES)
def test_sdf_reg(n, off):
    g = np.random.default_rng(200 + n % 1000)
    sdf, sg = g.standard_normal(n).astype(np.float32), g.standard_normal(n).astype(np.float32)
    grad, gg = g.standard_normal((n, 3)).astype(np.float32), g.standard_normal((n, 3)).astype(np.float32)
    w_sdf, w_grad = 200.0, 0.25

    def operand(a):                                   # `off` floats past a 16-byte boundary
        return Window(1, a.size, a.size + off, off, a.reshape(1, -1))
    ins = [operand(a) for a in (sdf, grad, sg, gg)]
    (ref_g, ref_s), want_ds, want_dg = T.sdf_reg(sdf, grad, sg, gg, w_sdf, w_grad)
    for null in (None, 'dsdf', 'dgrad'):
        ds, dg = Window(1, n, n + off, off), Window(1, 3 * n, 3 * n + off, off)
        sums = _sums()
        _call('ofx_sdf_reg_loss', ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, n, w_sdf, w_grad, sums.data_ptr(),
              None if null == 'dsdf' else ds.ptr, None if null == 'dgrad' else dg.ptr)
        got = sums.cpu().numpy()
        for k, ref in ((0, ref_g), (1, ref_s)):
            total = FILL[k] + ref
            print('sdf_reg n %d sums[%d]: relative difference %.3e (bound %.3e)'
                  % (n, k, abs(got[k] - total) / total, n * 2.0 ** -52))
            assert abs(got[k] - total) <= n * 2.0 ** -52 * total
        if null == 'dsdf':
            assert ds.untouched()
        else:
            assert np.array_equal(_bits(ds.get().reshape(-1)), _bits(want_ds))
        if null == 'dgrad':
            assert dg.untouched()
        else:
            assert np.array_equal(_bits(dg.get().reshape(-1)), _bits(want_dg.reshape(-1)))
        if n > 65537 and null is None:
            break                                     # the NULL outputs take no other path at the largest size


def test_sdf_reg_refusals():
    n = 32
    bufs = [Window(1, n * k, n * k, 0, np.ones((1, n * k), np.float32)) for k in (1, 3, 1, 3)]
    ds, dg, sums = Window(1, n, n), Window(1, 3 * n, 3 * n), _sums()
    ok = dict(sdf=bufs[0].ptr, grad=bufs[1].ptr, sg=bufs[2].ptr, gg=bufs[3].ptr, n=n, sums=sums.data_ptr())
    for bad in (dict(n=-1), dict(sums=None), dict(sums=None, n=0), dict(sdf=None), dict(grad=None), dict(sg=None),
                dict(gg=None)):
        a = dict(ok, **bad)
        _refused('ofx_sdf_reg_loss', a['sdf'], a['grad'], a['sg'], a['gg'], a['n'], 200.0, 0.25, a['sums'], ds.ptr, dg.ptr)
    _call('ofx_sdf_reg_loss', None, None, None, None, 0, 200.0, 0.25, sums.data_ptr(), None, None)       # nothing to read
    torch.cuda.synchronize()
    assert ds.untouched() and dg.untouched() and sums.cpu().tolist() == list(FILL)


# ------------------------------------------------------------------------------------------------ ofx_kl_sample_fwd / _bwd
KL_FILL = 0.25
# (E, n): n E = 2 097 152 + (257, 771, 1028, 2056): the grid-stride step runs; the small ones cover the block edges
KL_CASES = [(1, 0), (1, 1), (3, 85), (3, 86), (4, 64), (4, 65), (8, 8193), (1, STRIDE), (3, 699051 + 257), (4, 524288 + 257),
            (8, 262144 + 257)]


@pytest.mark.parametrize('layout', ['tight', 'pitched'])
@pytest.mark.parametrize('E,n', KL_CASES)
def test_kl(E, n, layout):
    ld, pcol, ldp, dcol = (2 * E, 0, 2 * E, 0) if layout == 'tight' else (2 * E + 3, 1, 2 * E + 1, 1)
    big = n * E > T.GRID_CAP
    params, noise, dz = T.posterior_case(n, E, 300 + E + n % 1000, hot=not big)
    assert not big or n * E - T.GRID_CAP >= 257
    pw = Window(n, 2 * E, ld, pcol, params)
    off = 0 if layout == 'tight' else 1
    nz, gz = Window(1, n * E, n * E + off, off, noise.reshape(1, -1)), Window(1, n * E, n * E + off, off, dz.reshape(1, -1))
    kl_scale = 0.1
    for with_noise in ((True,) if big and layout == 'pitched' else (True, False)):
        z = Window(1, n * E, n * E + off, off)
        kl = torch.tensor([KL_FILL], dtype=torch.float64, device=dev())
        _call('ofx_kl_sample_fwd', pw.ptr, ld, nz.ptr if with_noise else None, n, E, z.ptr, kl.data_ptr())
        (z_ref, S_z), (kl_ref, S_kl) = T.posterior(params, noise if with_noise else None, E)
        zg = z.get().reshape(n, E)
        if with_noise:
            used = assert_close(torch.tensor(zg), torch.tensor(z_ref), S_z, T.KL_C_Z, 'z E %d n %d' % (E, n))
        else:
            assert np.array_equal(_bits(zg), _bits(params[:, :E]))
            used = 0.0
        total, bound = float(kl_ref.sum()), T.KL_C_TERM * U * float(S_kl.sum()) + n * E * 2.0 ** -52 * (
            KL_FILL + float(np.abs(kl_ref).sum()))
        err = abs(float(kl) - KL_FILL - total)
        print('kl E %d n %d noise %s: z uses %.3f of its bound, kl sum %.9g |err| %.3e bound %.3e (%.3f)'
              % (E, n, with_noise, used, total, err, bound, err / bound if bound else 0.0))
        assert err <= bound
        # kl_sum NULL: the same z
        z2 = Window(1, n * E, n * E + off, off)
        _call('ofx_kl_sample_fwd', pw.ptr, ld, nz.ptr if with_noise else None, n, E, z2.ptr, None)
        assert np.array_equal(_bits(z2.get()), _bits(z.get()))
    for with_noise, with_dz in (((True, True),) if big and layout == 'pitched' else ((True, True), (False, True), (True, False))):
        dp = Window(n, 2 * E, ldp, dcol)
        _call('ofx_kl_sample_bwd', pw.ptr, ld, nz.ptr if with_noise else None, gz.ptr if with_dz else None, n, E,
              kl_scale, dp.ptr, ldp)
        (dm, S_m), (dl, S_l) = T.posterior_bwd(params, noise if with_noise else None, dz if with_dz else None, E, kl_scale)
        got = dp.get()
        u1 = assert_close(torch.tensor(got[:, :E]), torch.tensor(dm), S_m, T.KL_C_DMEAN, 'dmean E %d n %d' % (E, n))
        u2 = assert_close(torch.tensor(got[:, E:]), torch.tensor(dl), S_l, T.KL_C_DLV, 'dlogvar E %d n %d' % (E, n))
        blocked = (params[:, E:] < np.float32(T.LV_LO)) | (params[:, E:] > np.float32(T.LV_HI))
        assert np.all(_bits(got[:, E:][blocked]) == 0)                      # exactly +0 where the clamp blocks
        print('kl bwd E %d n %d noise %s dz %s: dmean uses %.3f, dlogvar %.3f of the bound' % (E, n, with_noise, with_dz,
                                                                                          u1, u2))


def test_kl_clamp_passes_at_its_bounds():
    """the gradient of the log-variance at exactly -30 and 20 is the closed form, one ulp outside it is 0"""
    sp = T.logvar_specials()
    params = np.stack([np.full(len(sp), 0.5, np.float32), sp], 1)
    noise, dz = np.full((len(sp), 1), 0.75, np.float32), np.full((len(sp), 1), -1.25, np.float32)
    pw, nz, gz = Window(len(sp), 2, 2, 0, params), Window(len(sp), 1, 1, 0, noise), Window(len(sp), 1, 1, 0, dz)
    dp = Window(len(sp), 2, 2)
    _call('ofx_kl_sample_bwd', pw.ptr, 2, nz.ptr, gz.ptr, len(sp), 1, 0.1, dp.ptr, 2)
    got = dp.get()[:, 1]
    (_, _), (dl, S_l) = T.posterior_bwd(params, noise, dz, 1, 0.1)
    assert_close(torch.tensor(got), torch.tensor(dl[:, 0]), S_l[:, 0], T.KL_C_DLV, 'dlogvar at the specials')
    passes = np.array([1, 1, 0, 1, 1, 0, 0, 0, 1], dtype=bool)
    assert np.all(got[passes] != 0) and np.all(_bits(got[~passes]) == 0)


def test_kl_refusals():
    E, n = 3, 16
    params, noise, dz = T.posterior_case(n, E, 9)
    pw, nz, gz = Window(n, 2 * E, 2 * E, 0, params), Window(n, E, E, 0, noise), Window(n, E, E, 0, dz)
    z, dp = Window(n, E, E), Window(n, 2 * E, 2 * E)
    kl = torch.tensor([KL_FILL], dtype=torch.float64, device=dev())
    ok = dict(params=pw.ptr, ld=2 * E, n=n, E=E, z=z.ptr, dp=dp.ptr, ldp=2 * E)
    for bad in (dict(n=-1), dict(E=0), dict(E=-2), dict(params=None), dict(z=None), dict(ld=2 * E - 1)):
        a = dict(ok, **bad)
        _refused('ofx_kl_sample_fwd', a['params'], a['ld'], nz.ptr, a['n'], a['E'], a['z'], kl.data_ptr())
    for bad in (dict(n=-1), dict(E=0), dict(params=None), dict(dp=None), dict(ld=2 * E - 1), dict(ldp=2 * E - 1)):
        a = dict(ok, **bad)
        _refused('ofx_kl_sample_bwd', a['params'], a['ld'], nz.ptr, gz.ptr, a['n'], a['E'], 0.1, a['dp'], a['ldp'])
    _call('ofx_kl_sample_fwd', None, 2 * E, None, 0, E, None, kl.data_ptr())          # nothing to read or write
    _call('ofx_kl_sample_bwd', None, 2 * E, None, None, 0, E, 0.1, None, 2 * E)
    torch.cuda.synchronize()
    assert z.untouched() and dp.untouched() and float(kl) == KL_FILL
