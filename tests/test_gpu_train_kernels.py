"""GPU tests of csrc/ofx_train.hip: the multi-tensor AdamW + EMA call against the per-tensor kernels (bit-equal: the
arithmetic is one set of device helpers, csrc/ofx_optim.h) and ofx_mse_grad against torch / numpy.

Tolerances.  Multi-tensor: none (torch.equal).  ofx_mse_grad: dy bit-equal to torch's two fp32 operations; the loss
within relative n * 2^-52 of numpy's fp64 mean of the same fp32 differences -- every term is an exact fp64 product of
two fp32 numbers and non-negative, so any summation order of n terms is within (n - 1) * 2^-53 of the exact sum, the
final division adds 2^-53, and numpy's pairwise sum is bounded the same way."""
import ctypes

import numpy as np
import pytest
import torch

from octfusion_amd import _lib, training as TR
from octfusion_amd._lib import OfxAdamRow, OfxError, call, lib, ptr, stream

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

GUARD = -12345.0


def dev():
    return torch.device('cuda:0')


class Holder(torch.nn.Module):
    def __init__(self, named):
        super().__init__()
        for k, v in named.items():
            self.register_parameter(k, torch.nn.Parameter(v, requires_grad=False))


class Arena:
    """One backing allocation filled with GUARD; tensors are carved out of it with >= 4 guard elements around each, at
    16-byte aligned offsets unless `skew` asks for a 4-byte offset (a view like base[1:1 + n])."""

    def __init__(self, sizes, skews=()):
        self.spans, off = [], 4
        for i, n in enumerate(sizes):
            start = off + (1 if i in skews else 0)
            self.spans.append((start, n))
            off = (start + n + 4 + 3) // 4 * 4
        self.buf = torch.full((off + 4,), GUARD, dtype=torch.float32, device=dev())
        assert self.buf.data_ptr() % 16 == 0

    def view(self, i):
        s, n = self.spans[i]
        return self.buf[s:s + n]

    def fill(self, values):
        for i, v in enumerate(values):
            self.view(i).copy_(v)
        return self

    def guards_intact(self):
        mask = torch.ones_like(self.buf, dtype=torch.bool)
        for s, n in self.spans:
            mask[s:s + n] = False
        return bool((self.buf[mask] == GUARD).all())


def test_multi_tensor_equals_the_per_tensor_kernels():
    c = lib().ofx_adamw_ema_multi_chunk()
    sizes = [1, 3, 7, 255, 256, 257, c - 1, c, c + 1, 3 * c + 5, 0] + [64] * 70      # 81 rows: crosses a 64-row slab
    T = len(sizes)
    names = ['t%02d' % i for i in range(T)]
    SKEW, NO_GRAD, NO_EMA = 5, 7, 8          # n = 257 as a 4-byte-offset view; n = c without gradient; c + 1 without EMA
    g0 = torch.Generator().manual_seed(17)
    init = [torch.randn(n, generator=g0) for n in sizes]
    ema_init = [torch.randn(n, generator=g0) for n in sizes]
    frozen_init, frozen_ema_init = torch.randn(1000, generator=g0), torch.randn(1000, generator=g0)
    grads_cpu = [[torch.randn(n, generator=g0) for n in sizes] for _ in range(3)]

    def setup():
        P = Arena(sizes, skews={SKEW}).fill(init)
        M, V, E = Arena(sizes).fill([torch.zeros(n) for n in sizes]), Arena(sizes).fill(
            [torch.zeros(n) for n in sizes]), Arena(sizes).fill(ema_init)
        F = Arena([1000, 1000]).fill([frozen_init, frozen_ema_init])
        assert P.view(SKEW).data_ptr() % 16 == 4
        net = Holder(dict({k: P.view(i) for i, k in enumerate(names)}, frozen=F.view(0)))
        ema = Holder(dict({k: E.view(i) for i, k in enumerate(names) if i != NO_EMA}, frozen=F.view(1)))
        opt = TR.AdamW({k: p for k, p in net.named_parameters() if k != 'frozen'}, lr=3e-3, weight_decay=0.1,
                       sync=False)
        opt.state = {k: (M.view(i), V.view(i)) for i, k in enumerate(names)}
        return dict(P=P, M=M, V=V, E=E, F=F, net=net, ema=ema, opt=opt)

    ref, fus = setup(), setup()
    assert all(p.data_ptr() == ref['P'].view(i).data_ptr() for i, p in enumerate(list(ref['net'].parameters())[:T]))
    # what ema_update pairs up: the live parameters that have an EMA twin, in the EMA module's order
    ref_live = Holder({k: p.data for k, p in ref['net'].named_parameters() if k in dict(ref['ema'].named_parameters())})
    versions = {k: p._version for k, p in fus['net'].named_parameters()}
    for step in range(3):
        grads = {k: grads_cpu[step][i].to(dev()) for i, k in enumerate(names) if i != NO_GRAD}
        ref['opt'].step(dict(grads))
        TR.ema_update(ref['ema'], ref_live, 0.9)
        fus['opt'].step(dict(grads), ema=fus['ema'], ema_rate=0.9, fused=True, source=fus['net'])
    torch.cuda.synchronize()
    for key in ('P', 'M', 'V', 'E', 'F'):
        a, b = ref[key], fus[key]
        for i, (_, n) in enumerate(a.spans):
            assert torch.equal(a.view(i), b.view(i)), (key, i, n)
        assert a.guards_intact() and b.guards_intact(), key
    # the rows moved at all, and the special rows did what the rules say
    P, M, V, E, F = (fus[k] for k in ('P', 'M', 'V', 'E', 'F'))
    assert not torch.equal(P.view(9).cpu(), init[9]) and not torch.equal(E.view(9).cpu(), ema_init[9])
    assert torch.equal(P.view(NO_GRAD).cpu(), init[NO_GRAD])                 # no gradient: parameter and moments untouched
    assert not M.view(NO_GRAD).any() and not V.view(NO_GRAD).any()
    assert not torch.equal(E.view(NO_GRAD).cpu(), ema_init[NO_GRAD])         # ... only the EMA moved
    assert torch.equal(E.view(NO_EMA).cpu(), ema_init[NO_EMA])               # no EMA row: AdamW only
    assert not torch.equal(P.view(NO_EMA).cpu(), init[NO_EMA])
    assert torch.equal(F.view(0).cpu(), frozen_init) and not torch.equal(F.view(1).cpu(), frozen_ema_init)
    # written tensors were version-bumped (packed-weight caches key on it; the views of one arena share a counter)
    assert all(p._version > versions[k] for k, p in fus['net'].named_parameters() if k != 'frozen')
    assert all(p._version > 0 for p in fus['ema'].parameters())
    # against the closed form on one small row, so that both paths being wrong the same way would show
    p, m, v, e = init[2].double(), torch.zeros(7).double(), torch.zeros(7).double(), ema_init[2].double()
    for step in range(3):
        g = grads_cpu[step][2].double()
        p = p * (1 - 3e-3 * 0.1)
        m, v = 0.9 * m + 0.1 * g, 0.999 * v + 0.001 * g * g
        p = p - 3e-3 / (1 - 0.9 ** (step + 1)) * m / ((v / (1 - 0.999 ** (step + 1))).sqrt() + 1e-8)
        e = e * 0.9 + 0.1 * p
    torch.testing.assert_close(P.view(2).cpu().double(), p, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(E.view(2).cpu().double(), e, rtol=1e-5, atol=1e-6)


def test_multi_tensor_rejects_invalid_arguments():
    x, g, m, v = (torch.zeros(8, device=dev()) for _ in range(4))
    good = (ptr(x), ptr(g), ptr(m), ptr(v), None, 8)
    scal = (1e-3, 0.9, 0.999, 1e-8, 0.0)

    def run(rows, step=1, n_rows=None):
        table = (OfxAdamRow * max(len(rows), 1))(*rows)
        call('ofx_adamw_ema_multi', table, len(rows) if n_rows is None else n_rows, *scal, step, 0.9, stream())
    run([good])
    run([])
    run([(None, None, None, None, None, 0)])                       # n == 0: skipped, whatever the pointers
    for rows, kw in (([good], dict(step=0)),
                     ([(ptr(x), ptr(g), ptr(m), ptr(v), None, -1)], {}),
                     ([(None, ptr(g), ptr(m), ptr(v), None, 8)], {}),
                     ([(ptr(x), ptr(g), None, ptr(v), None, 8)], {}),
                     ([(ptr(x), ptr(g), ptr(m), None, None, 8)], {}),
                     ([good], dict(n_rows=-1))):
        with pytest.raises(OfxError, match='invalid argument'):
            run(rows, **kw)
    with pytest.raises(OfxError, match='invalid argument'):
        call('ofx_adamw_ema_multi', None, 2, *scal, 1, 0.9, stream())
    # a list that fails on its second row launches nothing for the first either
    w, one = torch.ones(8, device=dev()), torch.ones(8, device=dev())
    with pytest.raises(OfxError, match='invalid argument'):
        run([(ptr(w), ptr(one), ptr(m), ptr(v), None, 8), (None, None, None, None, ptr(x), 4)])
    torch.cuda.synchronize()
    assert torch.equal(w, one) and not x.any()


def mse(y, t):
    return TR.mse_grad(y, t)


@pytest.mark.parametrize('n', [1, 5, 255, 257, 65537])
def test_mse_grad(n):
    g = torch.Generator().manual_seed(n)
    y, t = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.5
    loss, dy = mse(y.to(dev()), t.to(dev()))
    assert loss.dtype == torch.float64 and loss.dim() == 0 and loss.is_cuda
    assert torch.equal(dy.cpu(), (y - t) * (2.0 / n))
    diff = (y.numpy() - t.numpy()).astype(np.float32)
    ref = float(np.mean(diff.astype(np.float64) ** 2))
    got = float(loss)
    print('n %d: loss %.17g, numpy %.17g, relative difference %.3e (bound %.3e)'
          % (n, got, ref, abs(got - ref) / ref, n * 2.0 ** -52))
    assert abs(got - ref) <= n * 2.0 ** -52 * ref
    again, dy2 = mse(y.to(dev()), t.to(dev()))
    assert torch.equal(again.view(torch.int64), loss.view(torch.int64)) and torch.equal(dy2, dy)
    zero, dz = mse(y.to(dev()), y.to(dev()).clone())
    assert float(zero) == 0.0 and not dz.any()


def test_mse_grad_on_unaligned_views_and_bad_arguments():
    n = 4101
    g = torch.Generator().manual_seed(2)
    yb, tb = torch.randn(n + 1, generator=g).to(dev()), torch.randn(n + 1, generator=g).to(dev())
    y, t = yb[1:], tb[1:]                                          # 4-byte offset: the element-wise path
    assert y.data_ptr() % 16 == 4
    dy = torch.full((n + 8,), GUARD, device=dev())
    partials = torch.empty(lib().ofx_mse_grad_partials(n), dtype=torch.float64, device=dev())
    loss = torch.empty((), dtype=torch.float64, device=dev())
    call('ofx_mse_grad', ptr(y), ptr(t), ptr(dy[4:]), ptr(partials), ptr(loss), n, stream())
    assert torch.equal(dy[4:4 + n], (y - t) * (2.0 / n))
    assert bool((dy[:4] == GUARD).all()) and bool((dy[4 + n:] == GUARD).all())
    ref, _ = mse(y.clone(), t.clone())                             # the aligned path: same differences, other order
    assert abs(float(loss) - float(ref)) <= n * 2.0 ** -52 * float(ref)
    for args in ((ptr(y), ptr(t), ptr(dy), ptr(partials), ptr(loss), 0),
                 (None, ptr(t), ptr(dy), ptr(partials), ptr(loss), 4),
                 (ptr(y), ptr(t), ptr(dy), None, ptr(loss), 4),
                 (ptr(y), ptr(t), ptr(dy), ptr(partials), None, 4)):
        with pytest.raises(OfxError, match='invalid argument'):
            call('ofx_mse_grad', *args, stream())
    assert isinstance(ctypes.sizeof(OfxAdamRow), int) and ctypes.sizeof(OfxAdamRow) == 48
    assert _lib.lib().ofx_mse_grad_partials(0) == 0
