"""ofx_graphconv_narrow_in, ofx_graphconv_narrow_in_tab, ofx_narrow_out_pack, ofx_narrow_out_type_term and
ofx_graphconv_narrow_out (csrc/ofx_narrow.hip) one call at a time through the C ABI, with raw framed buffers, off the
shipped shapes: every template instantiation of the two input kernels (K <= 64 / <= 72 / <= 96, cin <= 4 / <= 8), both
output widths, row counts around the 64-row group, one persistent launch in which every block walks at least three groups
(a stage of the two-stage LDS buffer is reused) with batch labels cut inside groups, odd and unaligned x, wide pitches,
statistics with uniform and mixed groups and an exactly sized workspace, segments of 255 rows of one node type (the stated
limit of _tab), 256 and 1000 rows (narrow_in), every cout of the output side and every OFX_EINVAL clause.  The reference is
the float64 restatement of tests/gconv_entry_oracle.py, every comparison elementwise against its derived bounds
(tests/test_gconv_entry_oracle.py: they admit honest fp32 arithmetic and reject the planted errors, the byte-wide type
counter among them).  Framing as in tests/test_gpu_gconv_entry.py."""
import numpy as np
import pytest
import torch

import gconv_entry_oracle as O
import gemm_oracle as GM
import graph_oracle as GR
from test_gpu_fullwidth import dev
from test_gpu_gconv_entry import _L, _Out, _Stats, _bits, _f32, _status
from test_gpu_gconv_planes_entry import _frame_u8, _i32

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

COVER = {}
WORST = {}
IN_ARGS = ('x', 'ldx', 'cin', 'n', 'seg_ptr', 'col', 'ntype', 'nt', 'W', 'cout', 'bias', 'bid', 'out', 'ldc', 'stats', 'stats_ld',
           'ws', 'ws_bytes')
TAB_ARGS = IN_ARGS[:6] + ('ext', 'multi', 'n_multi', 'aux') + IN_ARGS[6:]


def _cover(*k):
    COVER[k] = COVER.get(k, 0) + 1


def _worst(k, w):
    WORST[k] = max(WORST.get(k, 0.0), w)


def _odd_ld(cin):
    return cin + 1 if cin % 2 == 0 else cin + 2


def _narrow_in(c, r, tab, what, bias=True, stats=False, x_off=4, ldc=None, stats_ld=None, ws_short=0, multi=True, override=None):
    """One launch of ofx_graphconv_narrow_in (tab=False) or _tab on the operands of c; returns the status string"""
    L = _L()
    ldx, ldc, sld = _odd_ld(c.cin), ldc or c.cout + 4, stats_ld or c.cout + 3
    V = len(c.multi)
    keep = [_f32(c.x, ldx, x_off), _f32(c.W), _f32(c.bias)]
    tabs = [_i32(t) for t in (c.seg_ptr, c.col, c.ext.reshape(-1), c.multi, c.bid)]
    tbuf, ts = _frame_u8(torch.from_numpy(c.node_type))
    out = _Out(c.n, c.cout, ldc)
    a = dict(x=keep[0][1], ldx=ldx, cin=c.cin, n=c.n, seg_ptr=tabs[0].data_ptr(), col=tabs[1].data_ptr(),
             ntype=tbuf.data_ptr() + ts, nt=c.nt, W=keep[1][1], cout=c.cout, bias=keep[2][1] if bias else None, bid=None,
             out=out.ptr, ldc=ldc, stats=None,
             stats_ld=sld, ws=None, ws_bytes=0, ext=tabs[2].data_ptr(), multi=tabs[3].data_ptr() if multi else None, n_multi=V)
    rec = 32 if c.cin <= 4 else 64
    abuf, astart = _frame_u8(torch.full(((c.n + V + 1) * rec,), 0xFF, dtype=torch.uint8))
    a['aux'] = abuf.data_ptr() + astart
    st = wsbuf = None
    if stats:
        st = _Stats(c.B, c.cout, sld)
        nbytes = GM.cdiv(c.n, 64) * c.cout * 8
        wsbuf, wstart = _frame_u8(torch.full((nbytes,), 0xFF, dtype=torch.uint8))
        a.update(stats=st.ptr, bid=tabs[4].data_ptr(), ws=wsbuf.data_ptr() + wstart, ws_bytes=nbytes - ws_short)
    a.update(override or {})
    name = 'ofx_graphconv_narrow_in_tab' if tab else 'ofx_graphconv_narrow_in'
    rc = getattr(L.lib(), name)(*[a[k] for k in (TAB_ARGS if tab else IN_ARGS)], L.stream())
    torch.cuda.synchronize()
    what = '%s %s' % (name[4:], what)
    if override or ws_short:
        assert out.untouched(), what + ': a refused call wrote `out`'
        return _status(rc)
    assert rc == 0, (what, _status(rc))
    KP, CI = O.narrow_inst(c.cin, c.nt, tab)
    rr = dict(r, written=torch.ones(c.n, dtype=torch.bool))
    _worst(name[4:], out.check(rr, O.bound_narrow_in(r, KP), what))
    ah = abuf.cpu()
    assert bool((ah[:astart] == 0xFF).all()) and bool((ah[astart + (c.n + V + 1) * rec:] == 0xFF).all()), what + ': aux frame'
    assert tab or bool((ah == 0xFF).all())
    if stats:
        st.check(out.y, c.bid, 'narrow', what)
        wh = wsbuf.cpu()
        assert bool((wh[:wstart] == 0xFF).all()) and bool((wh[wstart + nbytes:] == 0xFF).all()), what + ': wrote past ws'
    _cover(name[4:], KP, CI, c.cout)
    return 'ok'


_REF = {}


def _case(key, *a, **kw):
    if key not in _REF:
        c = O.make_narrow_in(*a, **kw)
        _REF[key] = (c, O.reference_narrow_in(c), O.reference_narrow_in(c, bias=False))
    return _REF[key]


@pytest.mark.parametrize('width', O.NARROW_IN_WIDTHS, ids=lambda w: '%d-%d' % w)
def test_narrow_in_every_instantiation(width):
    """both entries on the same operands; n around the 64-row group; cout 64 and 128; bias on and off; an odd ldx > cin
    with x 4 bytes off a 16-B boundary; ldc > cout; statistics with stats_ld > cout and a workspace of exactly
    ceil(n / 64) * cout * 8 bytes, uniform and mixed groups"""
    cin, nt = width
    wi = O.NARROW_IN_WIDTHS.index(width)
    for i, n in enumerate(O.NARROW_NS):
        cout = 64 if (i + wi) % 2 else 128
        cuts = [0, 64, 100, 200] if n == 200 else None
        c, r, r0 = _case((cin, nt, n, cout), n, cin, nt, cout, 100 * wi + n, cuts=cuts)
        for tab in (False, True):
            what = 'cin %d nt %d n %d cout %d' % (cin, nt, n, cout)
            _narrow_in(c, r, tab, what, stats=True)
            _narrow_in(c, r0, tab, what + ' no bias', bias=False, x_off=0)
            if n == 200:
                _cover('stats', 'tab' if tab else 'csr', 'uniform + mixed groups')
                assert _narrow_in(c, r, tab, what, stats=True, ws_short=1) == 'invalid argument'


def test_narrow_in_refusals():
    c, r, _ = _case('refuse', 65, 3, 5, 64, 5)
    for tab in (False, True):
        for cin, nt in O.NARROW_IN_REFUSED:
            assert _narrow_in(c, r, tab, 'K = 98', override=dict(cin=cin, nt=nt, ldx=16)) == 'invalid argument'
        for ov in (dict(x=None), dict(seg_ptr=None), dict(col=None), dict(W=None), dict(cin=0), dict(cin=9), dict(ldx=2),
                   dict(nt=-1), dict(nt=9), dict(ntype=None), dict(cout=96), dict(ldc=63), dict(n=-1)):
            assert _narrow_in(c, r, tab, str(ov), override=ov) == 'invalid argument', (tab, ov)
        for ov in (dict(bid=None), dict(stats_ld=63), dict(ws=None)):
            assert _narrow_in(c, r, tab, str(ov), stats=True, override=ov) == 'invalid argument', (tab, ov)
    aux8 = _frame_u8(torch.zeros(1 << 16, dtype=torch.uint8))
    for ov in (dict(ext=None), dict(aux=None), dict(aux=aux8[0].data_ptr() + aux8[1] + 8), dict(n_multi=-1), dict(multi=None)):
        assert _narrow_in(c, r, True, str(ov), override=ov) == 'invalid argument', ov
    assert len(c.multi) > 0


def test_narrow_in_segment_sizes():
    """both entries: sizes 0 / 1 / 2 / 8 / 9 / 3 plus one segment of 255 rows of a single node type (the most _tab's byte
    counters hold); narrow_in alone: 256 and 1000 rows; _tab with n_multi = 0 and multi_seg NULL"""
    c, r, _ = _case('255', 300, 3, 5, 64, 7, sizes=O.SIZES + (255,), one_type=255)
    s = int(np.nonzero(np.diff(c.seg_ptr) == 255)[0][0])
    assert set(c.node_type[c.col[c.seg_ptr[s]:c.seg_ptr[s + 1]]].tolist()) == {0}
    for tab in (False, True):
        _narrow_in(c, r, tab, '255 of one type', stats=True)
    c, r, _ = _case('256', 300, 8, 2, 128, 8, sizes=(0, 1, 2, 256, 1000, 3), one_type=256)
    _narrow_in(c, r, False, '256 and 1000', stats=True)
    c, r, _ = _case('nomulti', 129, 4, 6, 64, 9, sizes=(0, 1, 1))
    assert len(c.multi) == 0
    _narrow_in(c, r, True, 'n_multi 0', multi=False)
    _narrow_in(c, r, False, 'n_multi 0')


def test_narrow_in_tab_every_block_walks_three_groups():
    """n = 64 * (3 * 2 * CUs) + 17: the persistent launch has 2 * CUs blocks, every block walks at least three row groups
    and stores into an LDS stage it has used before; batch labels cut inside groups"""
    cus = torch.cuda.get_device_properties(dev()).multi_processor_count
    n = 64 * (3 * 2 * cus) + 17
    assert n <= 110000
    cuts = [0, 1000, 64 * 777 + 13, n - 5, n]
    c, r, _ = _case('big', n, 3, 5, 64, 11, cuts=cuts)
    assert GM.cdiv(n, 64) >= 3 * 2 * cus
    _narrow_in(c, r, True, 'three groups per block', stats=True)
    _cover('narrow_in_tab', 'stage reuse')


# ------------------------------------------------------------------------------------------------ output side
def test_narrow_out_pack():
    L = _L()
    for C in (1, 64):
        for nt in (0, 5):
            for cout in range(1, 9):
                W = GM.weight(7 * (C + nt), cout, C + nt + cout, 'plain')
                wb, wp = _f32(W)
                for pw in (7 * cout, 32, 64):
                    out = _Out(C, pw, pw)
                    rc = L.lib().ofx_narrow_out_pack(wp, C, nt, cout, pw, out.ptr, L.stream())
                    torch.cuda.synchronize()
                    if pw < 7 * cout:
                        assert _status(rc) == 'invalid argument' and out.untouched()
                        continue
                    assert rc == 0
                    want = O.pack_reference(W, C, nt, cout, pw)
                    out.check(dict(ref=want.double(), S=want.abs().double(), written=torch.ones(C, dtype=torch.bool)), 0.0,
                              'pack C %d nt %d cout %d pw %d' % (C, nt, cout, pw))
                    assert torch.equal(out.y, want), (C, nt, cout, pw)
                    _cover('pack', pw == 7 * cout)
    wb, wp = _f32(GM.weight(7, 1, 1))
    out = _Out(1, 8, 8)
    for a in ((None, 1, 0, 1, 8, out.ptr), (wp, 1, 0, 1, 8, None), (wp, 0, 0, 1, 8, out.ptr), (wp, 1, -1, 1, 8, out.ptr),
              (wp, 1, 0, 0, 8, out.ptr), (wp, 1, 0, 9, 64, out.ptr), (wp, 1, 0, 1, 6, out.ptr)):
        assert _status(L.lib().ofx_narrow_out_pack(*a, L.stream())) == 'invalid argument'
    assert out.untouched()


@pytest.mark.parametrize('cout', (1, 3, 4, 5, 8))
def test_narrow_out_type_term(cout):
    """nt 0 / 5 / 8, ldt > 7 nt, n 1 / 31 / 33; nt = 0 with a bias is the bias alone, without one zeros"""
    L = _L()
    C = 16
    for nt in (0, 5, 8):
        for n in (1, 31, 33):
            seg_ptr, col = GR.hand_csr(n + nt, n, sizes=O.SIZES)
            ty = (np.arange(n) % max(nt, 1)).astype(np.uint8)
            tf = torch.zeros(n, 0)
            if nt:
                tf = torch.from_numpy(GR.type_frac_fast(seg_ptr, col, ty, nt)[0]).reshape(n, 7 * nt).float()
            W = GM.weight(7 * (C + nt), cout, n + nt + cout)
            bias = GM.operand((cout,), 3 + cout)
            ldt = 7 * nt + 3
            keep = [_f32(W), _f32(bias), _f32(tf, ldt) if nt else (None, None)]
            for with_bias in (True, False):
                ref, b = O.type_term(tf, nt, W, C, cout, bias if with_bias else None)
                out = _Out(n, cout, cout)
                rc = L.lib().ofx_narrow_out_type_term(keep[2][1], ldt, nt, n, keep[0][1], C, cout,
                                                      keep[1][1] if with_bias else None, out.ptr, L.stream())
                torch.cuda.synchronize()
                assert rc == 0
                what = 'type term cout %d nt %d n %d bias %d' % (cout, nt, n, with_bias)
                rr = dict(ref=ref, S=ref.abs(), written=torch.ones(n, dtype=torch.bool))
                _worst('narrow_out_type_term', out.check(rr, b, what))
                if nt == 0:
                    want = bias.expand(n, cout) if with_bias else torch.zeros(n, cout)
                    assert torch.equal(_bits(out.y), _bits(want.contiguous())), what
                _cover('type_term', 4 if cout <= 4 else 8, nt)
    out = _Out(1, cout, cout)
    for a in ((None, 38, 5, 1, keep[0][1], C, cout, None, out.ptr), (keep[2][1], 34, 5, 1, keep[0][1], C, cout, None, out.ptr),
              (keep[2][1], 59, 8, 1, None, C, cout, None, out.ptr), (keep[2][1], 59, 8, 1, keep[0][1], C, cout, None, None),
              (keep[2][1], 59, 8, 1, keep[0][1], 0, cout, None, out.ptr), (keep[2][1], 59, 8, 1, keep[0][1], C, 9, None, out.ptr),
              (keep[2][1], 59, -1, 1, keep[0][1], C, cout, None, out.ptr),
              (keep[2][1], 59, 8, -1, keep[0][1], C, cout, None, out.ptr)):
        assert _status(L.lib().ofx_narrow_out_type_term(*a, L.stream())) == 'invalid argument'
    assert out.untouched()


@pytest.mark.parametrize('cout', range(1, 9))
def test_narrow_out(cout):
    """ldp 7 cout / 32 / 64 where admissible, type_term NULL and given, ldc > cout, n 1 / 31 / 33 / 100, segments of 256 and
    1000 rows"""
    L = _L()
    for n in (1, 31, 33, 100):
        seg_ptr, col = GR.hand_csr(n + cout, n, sizes=(0, 1, 2, 256, 1000, 3))
        sp, cl = _i32(seg_ptr), _i32(col)
        tt = GM.operand((n, cout), 70 + cout)
        tb, tp = _f32(tt)
        for ldp in (7 * cout, 32, 64):
            if ldp < 7 * cout:
                continue
            P = GM.operand((n, ldp), 80 + cout + ldp)
            pb, pp = _f32(P)
            for given in (True, False):
                ref, b, S = O.reference_narrow_out(P, cout, seg_ptr, col, tt if given else None)
                out = _Out(n, cout, cout + 3)
                rc = L.lib().ofx_graphconv_narrow_out(pp, ldp, cout, n, sp.data_ptr(), cl.data_ptr(), tp if given else None,
                                                      out.ptr, cout + 3, L.stream())
                torch.cuda.synchronize()
                assert rc == 0
                what = 'narrow_out cout %d n %d ldp %d tt %d' % (cout, n, ldp, given)
                _worst('graphconv_narrow_out', out.check(dict(ref=ref, S=S, written=torch.ones(n, dtype=torch.bool)), b, what))
                _cover('narrow_out', 4 if cout <= 4 else 8, given)
    out = _Out(n, cout, cout)
    ok = (pp, ldp, cout, n, sp.data_ptr(), cl.data_ptr(), None, out.ptr, cout)
    for i, v in ((0, None), (4, None), (5, None), (7, None), (2, 0), (2, 9), (1, 7 * cout - 1), (8, cout - 1), (3, -1)):
        a = list(ok)
        a[i] = v
        assert _status(L.lib().ofx_graphconv_narrow_out(*a, L.stream())) == 'invalid argument', (i, v)
    assert out.untouched()


# ------------------------------------------------------------------------------------------------ reporting
def test_coverage_table():
    """(runs after the cases of this module) every instantiation and branch was launched"""
    print('NARROW_ENTRY coverage:')
    for k in sorted(COVER, key=str):
        print('NARROW_ENTRY   %r: %d' % (k, COVER[k]))
    want_in = {(k, ci, co) for k in (64, 96) for ci in (4, 8) for co in (64, 128)}
    want_tab = {(k, ci, co) for k in (64, 72, 96) for ci in (4, 8) for co in (64, 128)}
    assert {k[1:] for k in COVER if k[0] == 'graphconv_narrow_in' and len(k) == 4} == want_in
    assert {k[1:] for k in COVER if k[0] == 'graphconv_narrow_in_tab' and len(k) == 4} == want_tab
    assert ('narrow_in_tab', 'stage reuse') in COVER
    assert {k[1] for k in COVER if k[0] == 'stats'} == {'tab', 'csr'}
    assert {k[1:] for k in COVER if k[0] == 'narrow_out'} == {(co, g) for co in (4, 8) for g in (True, False)}
    assert {k[1:] for k in COVER if k[0] == 'type_term'} == {(co, nt) for co in (4, 8) for nt in (0, 5, 8)}
    assert {k[1] for k in COVER if k[0] == 'pack'} == {True, False}


def test_zz_worst_ratio():
    print('NARROW_ENTRY worst ratio to the bound:', {k: round(v, 4) for k, v in sorted(WORST.items())})
    assert set(WORST) == {'graphconv_narrow_in', 'graphconv_narrow_in_tab', 'narrow_out_type_term', 'graphconv_narrow_out'}
    assert all(v <= 1.0 for v in WORST.values())
