"""The GroupNorm forward entry points of csrc/ofx_norm.hip one at a time, through the C ABI (so that no dispatch threshold
of octfusion_amd.ops can route a case around the kernel it names), against the float64 restatement of tests/gn_oracle.py:
ofx_gn_stats / ofx_gn_stats_acc, ofx_gn_finalize / _window, ofx_gn_apply (mean / rstd given and finalised in the launch),
ofx_gn_apply_planes without a plan (with and without aux rows) and ofx_gn_fused_rows under both settings of
ofx_set_gn_rows16 -- at the widths, pitches and row layouts include/ofx.h admits rather than the ones a shipped config
produces.  The sibling-octet launch and the block plan stay with tests/test_gpu_gn_oct.py.

Every bound is elementwise (|got - ref| <= c 2^-24 S, gn_oracle) with c derived next to its formula;
tests/test_gn_oracle.py shows on the host that the same bounds accept fp32 arithmetic on the same cases and reject
planted errors.  Every output lies inside a wider NaN- or sentinel-filled buffer that is checked afterwards; batch ids
are non-decreasing.  Each test prints the largest |got - ref| / (2^-24 S) it saw and the share of the bound it used."""
import pytest
import torch
import torch.nn.functional as F

import gn_oracle as O
from test_gpu_fullwidth import dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SENT = -12345.678
NAN = float('nan')
EINVAL = 'invalid argument'


def _call(name, *a):
    from octfusion_amd import _lib
    return _lib.call(name, *a, _lib.stream())


def _p(t, off=0):
    return t.data_ptr() + off


def _bits(t):
    t = t.contiguous()
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _units(got, ref, S):
    """largest |got - ref| / (2^-24 S) over the elements with S > 0"""
    got, ref, S = got.detach().cpu().double(), ref.cpu().double(), torch.as_tensor(S).cpu().double().expand_as(ref)
    ok = S > 0
    return float(((got - ref).abs()[ok] / (O.U * S[ok])).max()) if bool(ok.any()) else 0.0


class Peak:
    """the largest error of a test in units of 2^-24 S and as a share of its bound"""
    def __init__(self, name):
        self.name, self.units, self.used = name, 0.0, 0.0

    def check(self, got, ref, S, c, what):
        self.used = max(self.used, O.assert_close(got, ref, S, c, what))
        self.units = max(self.units, _units(got, ref, S))

    def show(self):
        print('GN_ENTRY %s: largest error %.2f x 2^-24 S, %.3f of the bound' % (self.name, self.units, self.used))


def _framed(data, pitch, col0, fill, pad=1):
    """(buffer, view): `data` [n, C] as the column slice at col0 of a `fill`ed [n + 2 pad, pitch] device buffer"""
    n, C = data.shape
    buf = torch.full((n + 2 * pad, pitch), fill, dtype=data.dtype)
    buf[pad:pad + n, col0:col0 + C] = data
    buf = buf.to(dev())
    return buf, buf[pad:pad + n, col0:col0 + C]


def _frame_intact(buf, n, C, col0, fill, pad=1):
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    keep[pad:pad + n, col0:col0 + C] = False
    return _same(buf[keep], torch.full_like(buf, fill)[keep])


def _bid_dev(bid):
    """the ids on the device, with one valid id of slack behind them (n = 0 must not become a NULL pointer)"""
    return torch.cat([bid, torch.zeros(1, dtype=torch.int32)]).to(dev())


# ------------------------------------------------------------------------------------------------ statistics
def _stats_case(peak, C, sizes, pitch, col0, seed, rpb=64):
    B, n = len(sizes), sum(sizes)
    x, bid = O.make_x(sizes, C, C // 4, seed)
    s, mag = O.sums(x, bid, B)
    cS, cQ = O.sums_c(O.stats_run(C, rpb))
    xbuf, xv = _framed(x, pitch, col0, NAN)
    bd = _bid_dev(bid)
    what = 'C %d %r pitch %d' % (C, sizes, pitch)
    for name in ('ofx_gn_stats', 'ofx_gn_stats_acc'):
        fill = torch.zeros(B, C, 2, dtype=torch.float64)
        frame = torch.full(((B + 2) * C * 2,), NAN, dtype=torch.float64)
        if name.endswith('acc'):
            fill = 3.25 + (torch.arange(B * C * 2, dtype=torch.float64) % 7).view(B, C, 2)
            frame[C * 2:(B + 1) * C * 2] = fill.reshape(-1)
        frame = frame.to(dev())
        # (the pointer from the frame: the view of an n = 0 case is empty and has none)
        _call(name, _p(xbuf, (pitch + col0) * 4), pitch, n, C, _p(bd), B, _p(frame, C * 2 * 8))
        got = frame[C * 2:(B + 1) * C * 2].view(B, C, 2).cpu()
        peak.check(got[:, :, 0], fill[:, :, 0] + s[:, :, 0], mag[:, :, 0], cS, name + ' sum ' + what)
        peak.check(got[:, :, 1], fill[:, :, 1] + s[:, :, 1], mag[:, :, 1], cQ, name + ' sum of squares ' + what)
        for b, nb in enumerate(sizes):                             # an empty element: zeroed / left at its fill, exactly
            assert nb > 0 or torch.equal(got[b], fill[b]), (name, what, b)
        assert bool(torch.isnan(frame[:C * 2]).all()) and bool(torch.isnan(frame[(B + 1) * C * 2:]).all()), what
    assert _same(xbuf, _framed(x, pitch, col0, NAN)[0])


@pytest.mark.parametrize('C', O.STATS_C)
def test_stats_layouts(C):
    """ofx_gn_stats, then ofx_gn_stats_acc on a buffer pre-filled with a known non-zero pattern (expected = fill +
    reference): n in {0, 1, 63, 64, 65, 257} at B = 3, a one-row and an empty element, boundaries inside a row pass and
    inside the four-loads-in-flight loop, seven elements inside one 64-row block; row pitch C and a column slice of a
    wider buffer.  64-row blocks: a thread sums ceil(64 / (256 / (C / 4))) rows in fp32 (gn_oracle.sums_c)."""
    peak = Peak('stats C %d' % C)
    for i, sizes in enumerate(O.STATS_LAYOUTS):
        _stats_case(peak, C, sizes, C, 0, 1000 * C + i)
        _stats_case(peak, C, sizes, C + 12, 8, 1000 * C + i)
    peak.show()


@pytest.mark.parametrize('C,n,rpb', O.STATS_BIG)
def test_stats_blocks_larger_than_64_rows(C, n, rpb):
    """gn_stats_rows by hand (gn_oracle.STATS_BIG): n = 4097, C = 256, B = 1 -> 65 chunks > cap 64: a block owns 128 rows
    and a thread 32; n = 8193, C = 1024, B = 1 -> 129 chunks > cap 64: a block owns 192 rows, all 192 summed by one
    thread in fp32.  The bound takes that run length from the case, not from the library."""
    assert (C, n, rpb) in ((256, 4097, 128), (1024, 8193, 192))
    peak = Peak('stats C %d n %d (%d-row blocks)' % (C, n, rpb))
    _stats_case(peak, C, (n,), C, 0, C + n, rpb)
    peak.show()


# ------------------------------------------------------------------------------------------------ finalize
def _finalize_case(peak, C, groups, count_eps, sizes, window=None):
    B = len(sizes)
    x, bid = O.make_x(sizes, C, groups, C + groups)
    s, _ = O.sums(x, bid, B)
    cnt = O.counts(sizes)
    lo, hi = window or (0, C)
    cpg = C // groups
    gw = (hi - lo) // cpg
    m, r = O.finalize(s[:, lo:, 0], s[:, lo:, 1], cnt, hi - lo, gw, O.EPS, count_eps)
    cm, cr = O.finalize_c(s[:, lo:, 0], s[:, lo:, 1], cnt, hi - lo, gw, O.EPS, count_eps)
    sd, cd = s.to(dev()), cnt.to(dev())
    mean = torch.full((B + 2, C), SENT, device=dev())
    rstd = torch.full((B + 2, C), SENT, device=dev())
    if window:
        _call('ofx_gn_finalize_window', _p(sd), _p(cd), B, C, groups, lo, hi, O.EPS, count_eps, _p(mean[1:]), _p(rstd[1:]))
    else:
        _call('ofx_gn_finalize', _p(sd), _p(cd), B, C, groups, O.EPS, count_eps, _p(mean[1:]), _p(rstd[1:]))
    what = 'C %d G %d count_eps %g window %r' % (C, groups, count_eps, window)
    peak.check(mean[1:B + 1, lo:hi], m, m.abs(), cm, 'mean ' + what)
    peak.check(rstd[1:B + 1, lo:hi], r, r, cr, 'rstd ' + what)
    for t in (mean, rstd):
        keep = torch.ones_like(t, dtype=torch.bool)
        keep[1:B + 1, lo:hi] = False
        assert _same(t[keep], torch.full_like(t, SENT)[keep]), what
    return mean[1:B + 1], rstd[1:B + 1], m, r


@pytest.mark.parametrize('count_eps', [O.EPS, 0.0])
def test_finalize(count_eps):
    """ofx_gn_finalize and ofx_gn_finalize_window on the oracle's float64 sums, so that only finalize is under test:
    channels per group 1, 2, 3, 4, 6, 32; count_eps = eps (with an element of count 0: mean 0, rstd 1 / sqrt(eps)) and 0;
    windows in the middle of C.  Bound: the fp32 rounding of each result (gn_oracle.finalize_c: 1 + < 0.01)."""
    peak = Peak('finalize count_eps %g' % count_eps)
    sizes = (5, 0, 40) if count_eps else (5, 3, 40)
    for C, cpgs in ((12, (1, 2, 3, 4, 6)), (96, (1, 2, 3, 4, 6, 32))):
        for cpg in cpgs:
            mean, rstd, m, r = _finalize_case(peak, C, C // cpg, count_eps, sizes)
            if count_eps:
                assert float(mean[1].abs().max()) == 0.0
                assert bool((rstd[1] == rstd[1, 0]).all()) and abs(float(rstd[1, 0]) * O.f32(O.EPS) ** 0.5 - 1) < 1e-6
    for C, groups, lo, hi in ((128, 32, 32, 96), (288, 48, 96, 192), (96, 96, 32, 64)):
        _finalize_case(peak, C, groups, count_eps, sizes, (lo, hi))
    peak.show()


# ------------------------------------------------------------------------------------------------ fp32 apply
def _apply_launches(x, bid, sizes, C, groups, w, b, act, count_eps, s, ldx, colx, ldo, colo):
    """ofx_gn_apply with mean / rstd from ofx_gn_finalize, and with both NULL: (out given, out finalised in the launch)"""
    B, n = len(sizes), len(bid)
    xbuf, xv = _framed(x, ldx, colx, NAN)
    bd, sd, cd = _bid_dev(bid), s.to(dev()), O.counts(sizes).to(dev())
    wd, bb = w.to(dev()), b.to(dev())
    mean, rstd = torch.empty(B, C, device=dev()), torch.empty(B, C, device=dev())
    _call('ofx_gn_finalize', _p(sd), _p(cd), B, C, groups, O.EPS, count_eps, _p(mean), _p(rstd))
    outs = []
    for given in (True, False):
        obuf, ov = _framed(torch.full((n, C), SENT), ldo, colo, SENT)
        _call('ofx_gn_apply', _p(xv), ldx, n, C, _p(bd), _p(mean) if given else None, _p(rstd) if given else None,
              None if given else _p(sd), None if given else _p(cd), groups, O.EPS, count_eps, _p(wd), _p(bb), O.ACT_ID[act],
              _p(ov), ldo)
        assert _frame_intact(obuf, n, C, colo, SENT), 'wrote outside the output'
        outs.append(ov.clone())
    return outs


@pytest.mark.parametrize('C', sorted(O.APPLY_CPG))
def test_apply_fp32(C):
    """ofx_gn_apply with mean / rstd given and finalised in the launch: bit-equal (include/ofx.h), both within bound of
    the oracle.  Channels per group 1, 2, 3, 4, 6 as C admits; n in {1, 63, 65, 200}; three and seven batch elements
    inside one block (a third element's rows take the fallback that derives each channel's group on its own -- mode 0,
    every cpg, widths with idle lanes: C = 12, 100); all three activations; ldx != C, ldo != C.  The sums are the
    oracle's: only the apply is under test (c = 5 + the mean's rounding over S, gn_oracle.apply_c)."""
    peak = Peak('apply fp32 C %d' % C)
    w, b = O.make_affine(C, C)
    k = 0
    for cpg in O.APPLY_CPG[C]:
        for li, sizes in enumerate(O.APPLY_LAYOUTS):
            x, bid = O.make_x(sizes, C, C // cpg, C + 10 * cpg + li)
            for act in ((None, 'silu', 'gelu') if li == 1 else ((None, 'silu', 'gelu')[k % 3],)):
                k += 1
                count_eps = O.EPS if k % 2 else 0.0
                ref, S, c, _, s = O.apply_reference(x, bid, sizes, C, C // cpg, w, b, act, count_eps)
                given, fin = _apply_launches(x, bid, sizes, C, C // cpg, w, b, act, count_eps, s, C + 8, 4, C + 4, 4)
                what = 'C %d cpg %d %r %s' % (C, cpg, sizes, act)
                assert _same(given, fin), 'in-launch finalize differs from ofx_gn_finalize + apply: ' + what
                peak.check(fin, ref, S, c, what)
    peak.show()


# ------------------------------------------------------------------------------------------------ planes
def _planes_launch(xv, ldx, n, C, bd, mean, rstd, sd, cd, groups, count_eps, wd, bb, act, mode, out_ptr, ldo_bytes,
                   graph=None, aux_ptr=None):
    seg, col, multi = graph if graph else (None, None, None)
    _call('ofx_gn_apply_planes', _p(xv), ldx, n, C, _p(bd), mean, rstd, sd, cd, groups, O.EPS, count_eps, _p(wd), _p(bb),
          O.ACT_ID[act], mode, out_ptr, ldo_bytes, _p(seg) if graph else None, _p(col) if graph else None,
          _p(multi) if graph else None, len(multi) if graph else 0, aux_ptr, None, 0)


def _merge(raw_view, ldp, n, C, mode):
    out = torch.full((n, C), SENT, device=dev())
    _call('ofx_planes_merge', _p(raw_view), ldp, n, C, mode, _p(out), C)
    return out


@pytest.mark.parametrize('mode,C', O.PLANES_CASES)
def test_apply_planes(mode, C):
    """ofx_gn_apply_planes without aux, both finalize variants (bit-equal), decoded by gn_oracle's decoders from the raw
    bytes: hi + lo within the apply's bound plus the format's representation error (gn_oracle.rep_c), the hi half
    alone within the format's rounding of the value (so [lo | hi] fails); pitch wider than the row; modes 2 and 3
    also in place (out == x); then ofx_planes_merge bit for bit against the decoder."""
    peak = Peak('apply planes mode %d C %d' % (mode, C))
    esz = 2 if mode == 1 else 4
    groups = C // 4
    w, b = O.make_affine(C, C)
    wd, bb = w.to(dev()), b.to(dev())
    for li, sizes in enumerate(O.PLANES_LAYOUTS):
        B, n = len(sizes), sum(sizes)
        x, bid = O.make_x(sizes, C, groups, C + mode + li)
        act = ('silu', 'gelu')[li]
        ref, S, c, _, s = O.apply_reference(x, bid, sizes, C, groups, w, b, act, O.EPS)
        c = c + O.rep_c(mode, S)
        bd, sd, cd = _bid_dev(bid), s.to(dev()), O.counts(sizes).to(dev())
        mean, rstd = torch.empty(B, C, device=dev()), torch.empty(B, C, device=dev())
        _call('ofx_gn_finalize', _p(sd), _p(cd), B, C, groups, O.EPS, O.EPS, _p(mean), _p(rstd))
        raws = []
        for place in (('out',) if mode == 1 else ('out', 'in')):
            for given in (True, False):
                stats = (_p(mean), _p(rstd), None, None) if given else (None, None, _p(sd), _p(cd))
                if place == 'out':
                    xbuf, xv = _framed(x, C + 4, 4, NAN)
                    ldo = C * esz + 128
                    obuf = torch.full((n + 2, ldo), 0xA5, dtype=torch.uint8, device=dev())
                    _planes_launch(xv, C + 4, n, C, bd, *stats, groups, O.EPS, wd, bb, act, mode, _p(obuf[1:]), ldo)
                    raw = obuf[1:n + 1]
                    assert bool((obuf[0] == 0xA5).all()) and bool((obuf[n + 1] == 0xA5).all()) and \
                        bool((raw[:, C * esz:] == 0xA5).all()), 'wrote outside the plane lines'
                else:
                    xbuf, xv = _framed(x, C, 0, SENT)
                    _planes_launch(xv, C, n, C, bd, *stats, groups, O.EPS, wd, bb, act, mode, _p(xv), C * 4)
                    raw = xbuf[1:n + 1].view(torch.uint8).view(n, C * 4)
                    ldo = C * 4
                    assert _same(xbuf[0], torch.full_like(xbuf[0], SENT)) and _same(xbuf[n + 1], xbuf[0])
                assert _p(raw) % 128 == 0
                raws.append(raw[:, :C * esz].clone())
                if given and place == 'out':
                    merged = _merge(raw, ldo, n, C, mode)
        for r in raws[1:]:
            assert _same(r, raws[0]), 'finalize variants / in-place launch differ in their bytes'
        host = raws[0].cpu()
        dec = O.decode(host, C, mode)
        what = 'mode %d C %d %r' % (mode, C, sizes)
        peak.check(dec, ref, S, c, what)
        if mode != 1:
            O.assert_close(O.decode_hi(host, C, mode), ref, S, c + O.HI_C[mode], 'hi half ' + what)
        assert torch.equal(merged.cpu().double(), dec), 'ofx_planes_merge and the decoder disagree'
    peak.show()


def test_apply_planes_aux_rows_without_a_plan():
    """one hand-made CSR (gn_oracle.aux_case: 130 rows, B = 2, C = 64, mode 3, segments of 2, 4, 5 and 9 sources in both
    batch elements, 19 aux rows = two aux blocks): aux row 0 is all zero bytes, the others within bound of the float64
    mean of the normalised source rows (gn_oracle.aux_c), the main rows as without aux, both finalize variants;
    out == x with aux is OFX_EINVAL."""
    from octfusion_amd import _lib
    peak = Peak('apply planes aux rows')
    seg, col, multi, bid, sizes = O.aux_case()
    C, mode, groups, act, n, B, V = 64, 3, 16, 'silu', 130, 2, 18
    assert len(multi) == V and (V + 1) > 256 // (C // 4)
    x, _ = O.make_x(sizes, C, groups, 130)
    w, b = O.make_affine(C, C)
    ref, S, c, _, s = O.apply_reference(x, bid, sizes, C, groups, w, b, act, O.EPS)
    aref, aS = O.aux_rows(ref, seg, col, multi), O.aux_rows(S, seg, col, multi)
    ac = O.aux_c(c, seg, col, multi) + O.rep_c(mode, aS)
    graph = (seg.to(dev()), col.to(dev()), multi.to(dev()))
    wd, bb, bd, sd, cd = w.to(dev()), b.to(dev()), _bid_dev(bid), s.to(dev()), O.counts(sizes).to(dev())
    mean, rstd = torch.empty(B, C, device=dev()), torch.empty(B, C, device=dev())
    _call('ofx_gn_finalize', _p(sd), _p(cd), B, C, groups, O.EPS, O.EPS, _p(mean), _p(rstd))
    xbuf, xv = _framed(x, C, 0, NAN)
    ldo = 384
    seen = []
    for given in (True, False):
        stats = (_p(mean), _p(rstd), None, None) if given else (None, None, _p(sd), _p(cd))
        obuf = torch.full((n + 2, ldo), 0xA5, dtype=torch.uint8, device=dev())
        abuf = torch.full((V + 3, ldo), 0xA5, dtype=torch.uint8, device=dev())
        _planes_launch(xv, C, n, C, bd, *stats, groups, O.EPS, wd, bb, act, mode, _p(obuf[1:]), ldo, graph, _p(abuf[1:]))
        for buf, rows in ((obuf, n), (abuf, V + 1)):
            assert bool((buf[0] == 0xA5).all()) and bool((buf[rows + 1] == 0xA5).all()) and \
                bool((buf[1:rows + 1, C * 4:] == 0xA5).all())
        main, aux = obuf[1:n + 1, :C * 4].cpu(), abuf[1:V + 2, :C * 4].cpu()
        assert not bool(aux[0].any()), 'aux row 0 is not all zero bytes'
        peak.check(O.decode(main, C, mode), ref, S, c + O.rep_c(mode, S), 'main rows')
        peak.check(O.decode(aux, C, mode)[1:], aref[1:], aS[1:], ac[1:], 'aux rows')
        seen.append((main, aux))
    assert torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][1], seen[1][1])
    # in place with aux: refused, nothing written
    xb2, xv2 = _framed(x, C, 0, SENT)
    abuf = torch.full((V + 1, C * 4), 0xA5, dtype=torch.uint8, device=dev())
    with pytest.raises(_lib.OfxError, match=EINVAL):
        _planes_launch(xv2, C, n, C, bd, _p(mean), _p(rstd), None, None, groups, O.EPS, wd, bb, act, mode, _p(xv2), C * 4,
                       graph, _p(abuf))
    assert _same(xb2, _framed(x, C, 0, SENT)[0]) and bool((abuf == 0xA5).all())
    peak.show()


# ------------------------------------------------------------------------------------------------ fused rows
def _fused_case(peak, C, groups, rows, B, seed, ldx, colx, ldo, colo, expect16):
    """both settings of ofx_set_gn_rows16, count_eps = eps against the oracle and count_eps = 0 also against
    torch.nn.functional.group_norm in float64"""
    sizes = (rows,) * B
    n, cpg = rows * B, C // groups
    x, bid = O.make_x(sizes, C, groups, seed)
    w, b = O.make_affine(C, C)
    cS, cQ = O.fused_c(rows, cpg)
    xbuf, xv = _framed(x, ldx, colx, NAN)
    wd, bb = w.to(dev()), b.to(dev())
    al16 = all(p % 16 == 0 for p in (_p(xv), _p(wd), _p(bb))) and ldx % 4 == 0 and ldo % 4 == 0 and colo % 4 == 0
    takes16 = al16 and cpg in (2, 4, 8, 16) and groups % (16 // cpg) == 0 and rows >= 2048
    assert takes16 == expect16, 'the case is no longer the path it was written for'
    act = 'silu'
    for count_eps in (O.EPS, 0.0):
        ref, S, c, _, _ = O.apply_reference(x, bid, sizes, C, groups, w, b, act, count_eps, cS, cQ)
        outs = {}
        for knob in (1, 0):
            _call_knob(knob)
            obuf, ov = _framed(torch.full((n, C), SENT), ldo, colo, SENT)
            _call('ofx_gn_fused_rows', _p(xv), ldx, rows, B, C, groups, O.EPS, count_eps, _p(wd), _p(bb), O.ACT_ID[act],
                  _p(ov), ldo)
            assert _frame_intact(obuf, n, C, colo, SENT), 'wrote outside the output'
            what = 'fused C %d G %d rows %d B %d knob %d count_eps %g' % (C, groups, rows, B, knob, count_eps)
            peak.check(ov, ref, S, c, what)
            outs[knob] = ov.clone()
        if count_eps == 0.0:
            t = F.silu(F.group_norm(x.double().view(B, rows, C).transpose(1, 2), groups, w.double(), b.double(), O.f32(O.EPS)))
            t = t.transpose(1, 2).reshape(n, C)
            _, _, ct, _, _ = O.apply_reference(x, bid, sizes, C, groups, w, b, act, 0.0, cS, cQ, slack=1.0)
            for knob in (1, 0):
                peak.check(outs[knob], t, S, ct, 'against torch group_norm, knob %d' % knob)


def _call_knob(on):
    from octfusion_amd import _lib
    _lib.call('ofx_set_gn_rows16', on)


@pytest.mark.parametrize('C,groups', O.FUSED_WIDTHS)
def test_fused_rows(C, groups):
    """ofx_gn_fused_rows called directly, ofx_set_gn_rows16 at 1 and at 0, rows in {2047, 2048, 2049, 2817, 3073} (below
    2048 and for channels per group 6 / 12 or 12 groups at cpg 2 the per-group kernel runs whatever the knob says; from
    2048 up the 16-channel kernel, whose four-in-flight loop and remainder loop both take rows at every one of these
    sizes), B in {1, 3}, strided input and output.  The statistics are the kernel's own: bound gn_oracle.fused_c."""
    cpg = C // groups
    sixteen = cpg in (2, 4, 8, 16) and groups % (16 // cpg) == 0
    peak = Peak('fused rows C %d G %d' % (C, groups))
    try:
        for rows, B in O.FUSED_CASES:
            _fused_case(peak, C, groups, rows, B, C + rows, C + 8, 4, C + 4, 4, sixteen and rows >= 2048)
    finally:
        _call_knob(1)
    peak.show()


@pytest.mark.parametrize('ldx,colx,ldo,colo', [(72, 1, 68, 4), (69, 0, 68, 4), (72, 4, 67, 0), (72, 4, 68, 3)])
def test_fused_rows_unaligned_operands_take_the_per_group_kernel(ldx, colx, ldo, colo):
    """a pointer or a pitch that is not 16-byte aligned at a shape the 16-channel kernel would otherwise take (C = 64,
    16 groups, 2048 rows): same bound"""
    peak = Peak('fused rows unaligned')
    try:
        _fused_case(peak, 64, 16, 2048, 1, ldx + colo, ldx, colx, ldo, colo, False)
    finally:
        _call_knob(1)
    peak.show()


# ------------------------------------------------------------------------------------------------ rejections
def _refused(name, base, table, outputs):
    """every row of `table` (argument overrides) must return OFX_EINVAL and leave `outputs` (tensor, clone) intact"""
    from octfusion_amd import _lib
    for over in table:
        args = dict(base)
        args.update(over)
        with pytest.raises(_lib.OfxError, match=EINVAL):
            _call(name, *args.values())
        for t, before in outputs:
            assert _same(t, before), (name, over)
    _call(name, *base.values())                                    # the unmodified call goes through ...
    assert not all(_same(t, before) for t, before in outputs), name        # ... and writes


def test_rejections():
    """for each entry point one table of invalid arguments: C not a multiple of 4, C > 1024, pitch < C or not a multiple
    of 4, misaligned x / out / w, batch_size 0, groups not dividing C, act = 3, planes C not a multiple of the chunk,
    plane pitch too small or not a multiple of 16, out not 128-byte aligned, bad window bounds: OFX_EINVAL, outputs
    untouched."""
    C, n, B = 64, 40, 2
    sizes = (15, 25)
    x, bid = O.make_x(sizes, C, 16, 9)
    s, _ = O.sums(x, bid, B)
    xd, bd, sd, cd = torch.cat([x, x], 1).to(dev()), _bid_dev(bid), s.to(dev()), O.counts(sizes).to(dev())
    w, b = (t.to(dev()) for t in O.make_affine(2 * C, 1))
    sums = torch.full((B * C * 2,), 7.0, dtype=torch.float64, device=dev())
    for name in ('ofx_gn_stats', 'ofx_gn_stats_acc'):
        base = dict(x=_p(xd), ldx=2 * C, n=n, C=C, bid=_p(bd), B=B, sums=_p(sums))
        _refused(name, base, [dict(C=6), dict(C=1028, ldx=1028), dict(ldx=C - 4), dict(ldx=2 * C + 2), dict(x=_p(xd, 4)),
                              dict(B=0), dict(n=-1), dict(C=0)], [(sums, sums.clone())])
    mean, rstd = torch.full((B, C), SENT, device=dev()), torch.full((B, C), SENT, device=dev())
    outs = [(mean, mean.clone()), (rstd, rstd.clone())]
    base = dict(sums=_p(sd), count=_p(cd), B=B, C=C, G=16, eps=O.EPS, ce=O.EPS, mean=_p(mean), rstd=_p(rstd))
    _refused('ofx_gn_finalize', base, [dict(G=7), dict(B=0), dict(G=0), dict(C=0)], outs)
    mean.fill_(SENT), rstd.fill_(SENT)
    base = dict(sums=_p(sd), count=_p(cd), B=B, C=C, G=16, lo=32, hi=64, eps=O.EPS, ce=O.EPS, mean=_p(mean), rstd=_p(rstd))
    _refused('ofx_gn_finalize_window', base, [dict(lo=32, hi=32), dict(lo=64, hi=32), dict(hi=96), dict(lo=-32), dict(lo=16),
                                              dict(hi=48), dict(G=7), dict(B=0), dict(C=60, G=20, lo=0, hi=32)], outs)
    _call('ofx_gn_finalize', _p(sd), _p(cd), B, C, 16, O.EPS, O.EPS, _p(mean), _p(rstd))
    out = torch.full((n, 2 * C), SENT, device=dev())
    for fin in (False, True):
        base = dict(x=_p(xd), ldx=2 * C, n=n, C=C, bid=_p(bd), mean=None if fin else _p(mean), rstd=None if fin else _p(rstd),
                    sums=_p(sd) if fin else None, count=_p(cd) if fin else None, G=16, eps=O.EPS, ce=O.EPS, w=_p(w), b=_p(b),
                    act=1, out=_p(out), ldo=2 * C)
        table = [dict(C=6), dict(C=1028, ldx=1028, ldo=1028), dict(ldx=C - 4), dict(ldo=C - 4), dict(ldx=2 * C + 2),
                 dict(ldo=2 * C + 2), dict(x=_p(xd, 4)), dict(out=_p(out, 4)), dict(w=_p(w, 4)), dict(b=_p(b, 4)), dict(act=3),
                 dict(act=-1)]
        table += [dict(G=7), dict(G=0), dict(sums=None)] if fin else [dict(rstd=None), dict(mean=_p(mean, 4))]
        out.fill_(SENT)
        _refused('ofx_gn_apply', base, table, [(out, out.clone())])
    for mode in (1, 2, 3):
        esz, chunk = (2, 64) if mode == 1 else (4, 32)
        po = torch.full((n + 1, 1024), 0xA5, dtype=torch.uint8, device=dev())
        base = dict(x=_p(xd), ldx=2 * C, n=n, C=C, bid=_p(bd), mean=_p(mean), rstd=_p(rstd), sums=None, count=None, G=16,
                    eps=O.EPS, ce=O.EPS, w=_p(w), b=_p(b), act=1, mode=mode, out=_p(po), ldo=1024, seg=None, col=None,
                    multi=None, V=0, aux=None, plan=None, left=0)
        table = [dict(C=C + chunk // 2), dict(C=chunk // 2), dict(C=1024 + chunk, ldx=2048, ldo=8192), dict(ldx=C - 4),
                 dict(ldx=2 * C + 2), dict(ldo=C * esz - 16), dict(ldo=C * esz + 8), dict(out=_p(po, 64)), dict(out=_p(po, 16)),
                 dict(x=_p(xd, 4)), dict(w=_p(w, 4)), dict(act=3), dict(mode=0), dict(mode=4), dict(rstd=None),
                 dict(aux=_p(po, 512))]              # aux without its CSR
        _refused('ofx_gn_apply_planes', base, table, [(po, po.clone())])
    out.fill_(SENT)
    base = dict(x=_p(xd), ldx=2 * C, rows=n // B, B=B, C=C, G=16, eps=O.EPS, ce=0.0, w=_p(w), b=_p(b), act=1, out=_p(out),
                ldo=2 * C)
    _refused('ofx_gn_fused_rows', base, [dict(G=7), dict(G=0), dict(ldx=C - 1), dict(ldo=C - 1), dict(act=3), dict(act=-1),
                                         dict(rows=0), dict(B=0), dict(C=0)], [(out, out.clone())])
