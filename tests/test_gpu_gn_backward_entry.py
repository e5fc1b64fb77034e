"""ofx_gn_backward (csrc/ofx_norm.hip) through the C ABI, against float64 autograd through the operation
(tests/train_oracle.gn_backward): y = act((x - m) r w + b) with m and r functions of x as gn_oracle.finalize states them,
count_eps included.  mean and rstd come from ofx_gn_stats + ofx_gn_finalize on the same x, as ops.group_norm_backward
calls them.  dx is a column window whose neighbours are sentinels; coef, dgamma and dbeta sit between sentinel bands.

    cases (test_backward)   C 4, 36, 96 (C / 4 does not divide 256), 256, 1024 (the largest accepted); groups 1, C and 32
                            where it divides C; act none / silu / gelu; rows per batch element (200, 0, 63, 1, 64, 65) and
                            seventy elements of one row (more than two inside one 64-row block) -- of two rows where a
                            group is one channel: one value has no variance, the case the inputs exclude --; operands
                            tight and pitched ldx = C + 4, ldy = C + 8, lddx = C + 12
    test_backward_big       (4100) rows at C = 4: gn_stats_rows hands a block 128 rows; (8200) rows at C = 1024: the
                            grid-stride step of the apply kernel
    test_backward_empty     n = 0, B = 2: dx untouched, dgamma = dbeta = 0, coef finite
    test_backward_count_eps count_eps = 0.5 on elements of 1 to 3 rows, 1 and 4 channels per group: the count_eps terms
                            of the coefficients are a visible fraction of dx (tests/test_train_oracle.py shows that an
                            oracle without them misses this bound by a wide margin)
    refusals (OFX_EINVAL)   each NULL, n < 0, C < 4, C % 4, C > 1024, groups < 1, C % groups, batch_size < 1, each ld < C,
                            each ld % 4, x / dy / dx 4 bytes off 16, act -1 and 3

Bound: |got - ref| <= c 2^-24 S elementwise, S_dx = |w r g| + |c2 x| + |c3 - c2 mu|, S of dgamma / dbeta the sum of the
absolute terms, c = max(8, 3 x the worst ratio of the float32 host evaluation train_oracle.gn_backward_f32 on the same
inputs) (train_oracle.gn_c says why it is measured on the host and not counted).  Every group of the inputs has |mean| <=
8 sigma (asserted): beyond that the fp32 rounding of the GIVEN mean, amplified by r^3, is the operation's conditioning and
not the kernel's.  No bit-equality between two launches: the sums are reduced with fp64 atomics.
"""
import numpy as np
import pytest
import torch

import gn_oracle as GN
import train_oracle as T
from glue_oracle import assert_close
from test_gpu_fullwidth import dev
from test_gpu_graph_tables import Guarded, _p, _up
from test_gpu_loss_entry import Window, _call

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)



class Case:
    """the operands of one call on the device; check() launches statistics, finalize and the backward and compares"""

    def __init__(self, sizes, C, groups, seed, pitched, count_eps=GN.EPS):
        self.sizes, self.C, self.groups, self.count_eps = sizes, C, groups, count_eps
        self.B, self.n = len(sizes), sum(sizes)
        self.x, self.dy, self.bid = T.gn_bwd_inputs(sizes, C, groups, seed)
        self.w, self.b = GN.make_affine(C, seed)
        n, B = self.n, self.B
        self.ldx, self.ldy, self.lddx = (C + 4, C + 8, C + 12) if pitched else (C, C, C)
        self.xw = Window(n, C, self.ldx, 4 if pitched else 0, self.x.numpy())
        self.dyw = Window(n, C, self.ldy, 4 if pitched else 0, self.dy.numpy())
        self.dxw = Window(n, C, self.lddx, 8 if pitched else 0)
        self.bd, self.cnt = _up(self.bid.numpy(), torch.int32), GN.counts(sizes).to(dev())
        self.wd, self.bbd = self.w.to(dev()), self.b.to(dev())
        self.mean, self.rstd = Guarded(B * C, torch.float32), Guarded(B * C, torch.float32)
        self.sums = torch.full((B * C * 2,), 123.0, dtype=torch.float64, device=dev())          # scratch: zeroed inside
        self.coef, self.dg, self.db = Guarded(B * C * 3, torch.float32), Guarded(C, torch.float32), Guarded(C, torch.float32)

    def args(self, act):
        return dict(x=self.xw.ptr, ldx=self.ldx, dy=self.dyw.ptr, ldy=self.ldy, n=self.n, C=self.C, bid=_p(self.bd),
                    B=self.B, count=self.cnt.data_ptr(), groups=self.groups, count_eps=self.count_eps, mean=self.mean.ptr,
                    rstd=self.rstd.ptr, w=self.wd.data_ptr(), bias=self.bbd.data_ptr(), act=GN.ACT_ID[act],
                    sums=self.sums.data_ptr(), coef=self.coef.ptr, dx=self.dxw.ptr, lddx=self.lddx, dgamma=self.dg.ptr,
                    dbeta=self.db.ptr)

    @staticmethod
    def launch(a):
        _call('ofx_gn_backward', a['x'], a['ldx'], a['dy'], a['ldy'], a['n'], a['C'], a['bid'], a['B'], a['count'],
              a['groups'], a['count_eps'], a['mean'], a['rstd'], a['w'], a['bias'], a['act'], a['sums'], a['coef'], a['dx'],
              a['lddx'], a['dgamma'], a['dbeta'])

    def statistics(self):
        _call('ofx_gn_stats', self.xw.ptr, self.ldx, self.n, self.C, _p(self.bd), self.B, self.sums.data_ptr())
        _call('ofx_gn_finalize', self.sums.data_ptr(), self.cnt.data_ptr(), self.B, self.C, self.groups, GN.EPS,
              self.count_eps, self.mean.ptr, self.rstd.ptr)

    def check(self, act, what):
        cond = T.gn_conditioning(self.x, self.bid, self.sizes, self.C, self.groups, GN.EPS, self.count_eps)
        assert cond <= 8.0, cond
        self.statistics()
        self.launch(self.args(act))
        ref = T.gn_backward(self.x, self.dy, self.bid, self.sizes, self.C, self.groups, self.w, self.b, act, GN.EPS,
                            self.count_eps)
        c_dx, c_dg, c_db, host = T.gn_c(ref, self.x, self.dy, self.bid, self.sizes, self.C, self.groups, self.w, self.b,
                                        act, GN.EPS, self.count_eps)
        u = [assert_close(torch.tensor(self.dxw.get()), ref['dx'], ref['S_dx'], c_dx, what + ' dx'),
             assert_close(torch.tensor(self.dg.get()), ref['dgamma'], ref['S_dgamma'], c_dg, what + ' dgamma'),
             assert_close(torch.tensor(self.db.get()), ref['dbeta'], ref['S_dbeta'], c_db, what + ' dbeta')]
        assert np.isfinite(self.coef.get()).all()
        print('%s: |mean| / sigma <= %.2f; c (dx, dgamma, dbeta) = %.1f, %.1f, %.1f from host ratios %.2f, %.2f, %.2f; '
              'error / bound: %.3f, %.3f, %.3f' % (what, cond, c_dx, c_dg, c_db, host[0], host[1], host[2],
                                                             u[0], u[1], u[2]))


@pytest.mark.parametrize('pitched', [False, True])
@pytest.mark.parametrize('rows', ['ragged', 'seventy'])
@pytest.mark.parametrize('C,groups', T.GN_WIDTHS)
def test_backward(C, groups, rows, pitched):
    sizes = T.gn_sizes(C, groups, rows)
    case = Case(sizes, C, groups, T.gn_seed(C, groups, sizes), pitched)
    for act in GN.ACT_ID:
        case.check(act, 'C %d groups %d %s %s %s' % (C, groups, rows, 'pitched' if pitched else 'tight', act))


@pytest.mark.parametrize('n,C,groups,act', [(4100, 4, 1, 'silu'), (8200, 1024, 32, 'gelu')])
def test_backward_big(n, C, groups, act):
    assert T.stats_rows(n, 1) > 64 and (C == 4 or n * (C // 4) > T.GRID_CAP)
    Case((n,), C, groups, n, True).check(act, 'C %d groups %d rows %d %s' % (C, groups, n, act))


def test_backward_empty():
    case = Case((0, 0), 8, 2, 3, True)
    case.statistics()
    Case.launch(case.args('silu'))
    torch.cuda.synchronize()
    assert case.dxw.untouched()
    assert np.all(case.dg.get() == 0) and np.all(case.db.get() == 0) and np.isfinite(case.coef.get()).all()


@pytest.mark.parametrize('C,groups', T.GN_COUNT_EPS_WIDTHS)
def test_backward_count_eps(C, groups):
    """elements of 1 to 3 rows at count_eps = 0.5: sum (x - mean) = mean count_eps and 1 / (count + count_eps) are far
    from 0 and 1 / count"""
    case = Case(T.GN_COUNT_EPS_SIZES, C, groups, T.gn_seed(C, groups, T.GN_COUNT_EPS_SIZES), True, count_eps=0.5)
    for act in GN.ACT_ID:
        case.check(act, 'count_eps 0.5 C %d groups %d %s' % (C, groups, act))


def test_backward_refusals():
    case = Case((5, 3), 8, 2, 7, True)
    case.statistics()
    ok = case.args('silu')
    bad = [{k: None} for k in ('x', 'dy', 'bid', 'count', 'mean', 'rstd', 'w', 'bias', 'sums', 'coef', 'dx', 'dgamma', 'dbeta')]
    bad += [dict(n=-1), dict(C=0, groups=1), dict(C=6, groups=2), dict(C=1028, groups=4, ldx=1028, ldy=1028, lddx=1028),
            dict(groups=0), dict(groups=-1), dict(groups=3), dict(B=0), dict(ldx=4), dict(ldy=4), dict(lddx=4), dict(ldx=10),
            dict(ldy=10), dict(lddx=10), dict(x=ok['x'] + 4), dict(dy=ok['dy'] + 4), dict(dx=ok['dx'] + 4), dict(act=-1),
            dict(act=3)]
    from octfusion_amd import _lib
    for b in bad:
        with pytest.raises(_lib.OfxError, match='invalid argument'):
            Case.launch(dict(ok, **b))
    torch.cuda.synchronize()
    assert case.dxw.untouched() and case.coef.untouched() and case.dg.untouched() and case.db.untouched()
