"""ofx_graphconv_fwd, ofx_graphconv_bwd_data, ofx_gridconv_fwd, ofx_gridconv_bwd_data and ofx_gather_mean
(csrc/ofx_gemm.hip) one call at a time through the C ABI, with raw framed buffers, so that no choice of octfusion_amd.ops
(ldc = stats_ld = cout, a contiguous 16-B aligned x, the 96 MB workspace, an aux sized by the caller's habit) can route a
case around the branch it names: the branch-free path and the col path with every trigger that moves a call from one to
the other, pitches wider than the rows, every epilogue, the three routes of the fused statistics on both epilogues with
batch labels cut inside a wave tile, inside a later col chunk and on a chunk boundary, weighted multi-row reverse
segments, every tap-table mode, and every OFX_EINVAL clause.  The reference is the float64 restatement of
tests/gconv_entry_oracle.py; every comparison is elementwise against the DERIVED bound of that module
(tests/test_gconv_entry_oracle.py shows on the host that it admits honest fp32 arithmetic and rejects the planted errors).
Every operand sits in a larger allocation with >= 256 bytes of NaN / 0xff on both sides; `out`, `stats` and `aux` sit in
sentinel frames that must come back bit-unchanged outside the written window.  The path of a call is OBSERVED: the same
call with ws = NULL succeeds on the branch-free path and is OFX_EINVAL, with `out` untouched, on the col path."""
import contextlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gconv_entry_oracle as O
import gemm_oracle as GM
import graph_oracle as GR
from test_gpu_fullwidth import dev
from test_gpu_gconv_planes_entry import _frame_f32, _frame_u8, _i32

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SENT = -12345.678
STAT_SENT = 777.25
WS_BYTES = 8 << 20
COVER = {}                         # (entry, precision, path, epilogue, split-K, statistics route) -> launches
EPI = {}                           # (precision, epilogue name) -> launches
WORST = {}                         # (entry, precision name) -> worst |got - ref| / bound
_DEV = {}
_PACK = {}
_SHARED = {}


def _L():
    from octfusion_amd import _lib
    return _lib


def _status(rc):
    return 'ok' if rc == 0 else _L().lib().ofx_status_string(rc).decode()


def _ws():
    """one workspace for the module, 256-B aligned, NaN-filled before every launch that is checked"""
    if 'ws' not in _SHARED:
        _SHARED['ws'] = torch.empty(WS_BYTES + 256, dtype=torch.uint8, device=dev())
    return _SHARED['ws']


@contextlib.contextmanager
def _precision(p):
    lib = _L().lib()
    was = lib.ofx_get_precision()
    try:
        _L().call('ofx_set_precision', p)
        yield
    finally:
        lib.ofx_set_precision(was)


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Out:
    """[n, cout] at pitch ldc, `off` bytes into a sentinel-filled buffer with >= 256 B of sentinel rows on each side"""

    def __init__(self, n, cout, ldc, off=0):
        self.n, self.cout, self.ldc, self.f0 = n, cout, ldc, off // 4
        self.pad = (GM.cdiv(64, ldc) + 4) // 4 * 4
        self.rows = n + 2 * self.pad
        self.dev = torch.full((self.rows * ldc + self.f0 + 4,), SENT, device=dev())
        assert self.dev.data_ptr() % 256 == 0
        self.ptr = self.dev.data_ptr() + self.pad * ldc * 4 + off

    def untouched(self):
        h = self.dev.cpu()
        return torch.equal(_bits(h), _bits(torch.full_like(h, SENT)))

    def check(self, r, bnd, what):
        h = self.dev.cpu()
        edge = torch.cat([h[:self.f0], h[self.f0 + self.rows * self.ldc:]])
        assert torch.equal(_bits(edge), _bits(torch.full_like(edge, SENT))), what + ': wrote in front of / behind the buffer'
        buf = h[self.f0:self.f0 + self.rows * self.ldc].view(self.rows, self.ldc)
        self.y = buf[self.pad:self.pad + self.n, :self.cout].clone()
        return O.check_window(buf, self.pad, self.cout, r, bnd, SENT, what)


class _Stats:
    def __init__(self, B, cout, ld):
        self.B, self.cout = B, cout
        self.h0 = torch.full((B + 2, ld, 2), STAT_SENT, dtype=torch.float64)
        self.h0[1:B + 1, :cout] = 0.0
        self.dev = self.h0.to(dev())
        self.ptr = self.dev.data_ptr() + ld * 2 * 8

    def check(self, y, bid, route, what):
        h = self.dev.cpu()
        got = h[1:self.B + 1, :self.cout].clone()
        h[1:self.B + 1, :self.cout] = 0.0
        assert torch.equal(h, self.h0), what + ': statistics slots beyond cout / outside [0, B) touched'
        s, _ = O.stats_sums(y, bid, self.B)
        bS, bQ = O.stats_bound(y, bid, self.B, route)
        dS, dQ = (got[:, :, 0] - s[:, :, 0]).abs(), (got[:, :, 1] - s[:, :, 1]).abs()
        w = max(float((dS / bS.clamp(min=1e-300)).max()), float((dQ / bQ.clamp(min=1e-300)).max()))
        print('GCONV_ENTRY %s: statistics (%s) worst %.3f of the bound' % (what, route, w))
        assert bool((dS <= bS).all()) and bool((dQ <= bQ).all()), what + ': fused statistics off (%s)' % route
        return w


class _Aux:
    """exactly (V + 1) * ld floats of NaN bytes in a 0xff frame; the kernel may write [V + 1, C] at pitch ld"""

    def __init__(self, V, C, ld, off=0):
        self.V, self.C, self.ld, self.nbytes = V, C, ld, (V + 1) * ld * 4
        self.dev, self.start = _frame_u8(torch.full((self.nbytes,), 0xFF, dtype=torch.uint8), off)
        self.ptr = self.dev.data_ptr() + self.start

    def rows(self, what):
        h = self.dev.cpu()
        idx = (torch.arange(self.V + 1)[:, None] * self.ld * 4 + torch.arange(self.C * 4)[None, :] + self.start).reshape(-1)
        win = torch.zeros(h.numel(), dtype=torch.bool)
        win[idx] = True
        assert bool((h[~win] == 0xFF).all()), what + ': wrote outside the (n_multi + 1) x cin window of aux'
        return h[idx].view(torch.float32).view(self.V + 1, self.C)

    def untouched(self):
        return bool((self.dev.cpu() == 0xFF).all())


def _f32(t, ld=None, off=0):
    """framed fp32 operand: (keep-alive buffer, pointer)"""
    t = t.reshape(1, -1) if t.dim() == 1 else t
    return _frame_f32(t, ld or t.shape[1], off)


def _pack(key, W, cin, nt, Kp, prec, conv3d=None):
    """ofx_pack_weights (GraphConv row permutation) / ofx_pack_conv3d under the precision in force, framed"""
    key = (key, prec)
    if key not in _PACK:
        L = _L()
        N = conv3d[1] if conv3d else W.shape[1]
        buf, s = _frame_u8(torch.zeros(L.lib().ofx_packed_floats(Kp, N) * 4, dtype=torch.uint8))
        Wd = W.contiguous().to(dev())
        if conv3d:
            L.call('ofx_pack_conv3d', Wd.data_ptr(), conv3d[0], conv3d[1], buf.data_ptr() + s, L.stream())
        else:
            L.call('ofx_pack_weights', Wd.data_ptr(), N, 1, W.shape[0], N, cin, nt, buf.data_ptr() + s, Kp, L.stream())
        torch.cuda.synchronize()
        _PACK[key] = (buf, buf.data_ptr() + s)
    return _PACK[key][1]


def _record(entry, prec, path, vec, split, route):
    k = (entry, prec, path, 'float4' if vec else 'scalar', bool(split), route)
    COVER[k] = COVER.get(k, 0) + 1


def _worst(entry, prec, w):
    k = (entry, O.PREC_NAME[prec])
    WORST[k] = max(WORST.get(k, 0.0), w)


# ------------------------------------------------------------------------------------------------ ofx_graphconv_fwd
FWD_ARGS = ('x', 'ldx', 'cin', 'n', 'nbr', 'seg_ptr', 'col', 'ext', 'multi', 'n_multi', 'aux', 'tf', 'ldt', 'nt_pad', 'Wp', 'Kp',
            'cout', 'bias', 'emb', 'lde', 'bid', 'res', 'ldr', 'out', 'ldc', 'stats', 'stats_ld', 'ws', 'ws_bytes')


def _upload(c, ldx, x_off, ldt):
    key = (id(c), ldx, x_off, ldt)
    if key not in _DEV:
        d = SimpleNamespace()
        d.xbuf, d.x = _f32(c.x, ldx, x_off)
        d.nbr, d.seg_ptr, d.col = _i32(c.nbr.reshape(-1)), _i32(c.seg_ptr), _i32(c.col)
        d.ext, d.multi, d.bid = _i32(c.ext.reshape(-1)), _i32(c.multi), _i32(c.bid)
        d.tfbuf, d.tf = _f32(c.tf, ldt) if c.nt_pad else (None, None)
        _DEV[key] = d
    return _DEV[key]


def _fwd_call(c, prec, o, ws, ws_bytes, ws_off=0):
    """one launch with fresh out / stats / aux frames"""
    L = _L()
    ldx, ldt = o.get('ldx') or c.cin, o.get('ldt') or c.nt_pad
    ldc, ldr, lde, sld = (o.get(k) or c.cout for k in ('ldc', 'ldr', 'lde', 'stats_ld'))
    d = _upload(c, ldx, o.get('x_off', 0), ldt)
    V = len(c.multi)
    f = SimpleNamespace(out=_Out(c.n, c.cout, ldc, o.get('out_off', 0)), keep=[])
    f.aux = _Aux(V, c.cin, ldx, o.get('aux_off', 0)) if o.get('aux', True) else None
    a = dict(x=d.x, ldx=ldx, cin=c.cin, n=c.n, nbr=d.nbr.data_ptr(), seg_ptr=d.seg_ptr.data_ptr(), col=d.col.data_ptr(),
             ext=d.ext.data_ptr() if o.get('ext', True) else None, multi=d.multi.data_ptr() if o.get('multi', True) else None,
             n_multi=V, aux=f.aux.ptr if f.aux else None, tf=d.tf, ldt=ldt, nt_pad=c.nt_pad,
             Wp=_pack(('fwd', id(c)), c.W, c.cin, c.nt, c.Kp, prec), Kp=c.Kp, cout=c.cout, bias=None, emb=None, lde=lde,
             bid=None, res=None, ldr=ldr, out=f.out.ptr, ldc=ldc, stats=None, stats_ld=sld, ws=None, ws_bytes=0)
    if o.get('bias', True):
        b, a['bias'] = _f32(c.bias)
        f.keep.append(b)
    if o.get('emb', True):
        b, a['emb'] = _f32(c.emb, lde)
        f.keep.append(b)
    if o.get('res', True):
        b, a['res'] = _f32(c.res, ldr)
        f.keep.append(b)
    if o.get('emb', True) or o.get('stats'):
        a['bid'] = d.bid.data_ptr()
    f.stats = _Stats(c.B, c.cout, sld) if o.get('stats') else None
    if f.stats:
        a['stats'] = f.stats.ptr
    if ws:
        _ws().fill_(0xFF)
        a['ws'], a['ws_bytes'] = _ws().data_ptr() + ws_off, ws_bytes
    a.update(o.get('override') or {})
    f.rc = L.lib().ofx_graphconv_fwd(*[a[k] for k in FWD_ARGS], L.stream())
    torch.cuda.synchronize()
    return f


def _fwd(c, r, prec, what, ws_bytes=WS_BYTES, ws_off=0, epi='all', **o):
    """The call twice: with ws = NULL (the path probe), then with the workspace; everything checked on the second."""
    o['bias'], o['emb'], o['res'] = O.EPILOGUES[epi]
    ldx = o.get('ldx') or c.cin
    fast = O.fast_path(c.cin, ldx, o.get('x_off', 0), o.get('ext', True), o.get('aux', True), o.get('aux_off', 0))
    what = '%s %s %s' % (what, O.PREC_NAME[prec], 'fast' if fast else 'col')
    with _precision(prec):
        p = _fwd_call(c, prec, o, False, 0)
        if fast:
            assert p.rc == 0, what + ': predicted the branch-free path, ws = NULL gave ' + _status(p.rc)
        else:
            assert _status(p.rc) == 'invalid argument' and p.out.untouched(), what + ': predicted the col path'
            assert p.aux is None or p.aux.untouched()
        f = _fwd_call(c, prec, o, True, ws_bytes, ws_off)
    assert f.rc == 0, (what, _status(f.rc))
    stats = bool(o.get('stats'))
    plans = O.launch_plan(fast, c.n, c.cout, c.Kp, ws_bytes, stats)
    ldc, ldr, lde = (o.get(k) or c.cout for k in ('ldc', 'ldr', 'lde'))
    vec = O.vec4(c.cout, ldc, o.get('out_off', 0), o['res'], ldr, 0, o['emb'], lde)
    w = f.out.check(r, O.bound(prec, r, plans), what)
    _worst('graphconv_fwd', prec, w)
    route = None
    if stats:
        route = O.stats_route(fast, c.n, c.cout, c.Kp, ws_bytes, vec, ws_off)
        f.stats.check(f.out.y, c.bid, route, what)
    if f.aux is not None:
        if fast:
            rows = f.aux.rows(what)
            mean, mag = O.seg_means(c.x, c.seg_ptr, c.col)
            idx = c.multi.long()
            assert bool((rows[0] == 0).all()), what + ': aux row 0 is not the zero row'
            err = (rows[1:].double() - mean[idx]).abs()
            assert bool((err <= O.mean_err(c.L.reshape(-1)[idx], mag[idx])).all()), what + ': aux means off'
        else:
            assert f.aux.untouched(), what + ': the col path wrote aux'
    _record('graphconv_fwd', prec, 'fast' if fast else 'col', vec, max(p_[2].nsplit for p_ in plans) > 1, route)
    EPI[(prec, epi)] = EPI.get((prec, epi), 0) + 1
    return f


_REF = {}


def _case(shape, epi='all', **kw):
    key = (shape[0], epi, str(sorted(kw.items())))
    if key not in _REF:
        c = O.case(shape, **kw)
        _REF[key] = (c, O.reference(c, *O.EPILOGUES[epi]))
    return _REF[key]


@pytest.mark.parametrize('prec', O.PRECISIONS)
@pytest.mark.parametrize('shape', O.FWD_SHAPES, ids=lambda s: s[0])
def test_graphconv_fwd_widths(shape, prec):
    """cin 32 / 64 (branch-free) and 3 / 24 (col), nt_pad 0 / 32 / 64, cout 3 / 36 / 64 / 130, n 1 / 63 / 129 / 300"""
    c, r = _case(shape)
    _fwd(c, r, prec, shape[0])


@pytest.mark.parametrize('prec', O.PRECISIONS)
@pytest.mark.parametrize('trig', O.TRIGGERS)
def test_graphconv_fwd_path_triggers(trig, prec):
    """a cin = 64 layer on the branch-free path, and each trigger alone that must send it to the col path"""
    c, r = _case(O.TRIGGER_SHAPE)
    kw = {'none': {}, 'no_ext': dict(ext=False), 'aux_null': dict(aux=False), 'aux_off': dict(aux_off=4), 'x_off': dict(x_off=4),
          'ldx': dict(ldx=c.cin + 2)}[trig]
    ldx = kw.get('ldx', c.cin)
    assert O.fast_path(c.cin, ldx, kw.get('x_off', 0), kw.get('ext', True), kw.get('aux', True), kw.get('aux_off', 0)) == \
        (trig == 'none')
    _fwd(c, r, prec, 'trigger ' + trig, **kw)


@pytest.mark.parametrize('prec', O.PRECISIONS)
@pytest.mark.parametrize('which', O.PITCHES)
def test_graphconv_fwd_pitches(which, prec):
    """every pitch wider than its rows, alone and together; ldx = cin + 32 stays on the branch-free path and aux holds
    exactly (n_multi + 1) * ldx floats (include/ofx.h)"""
    c, r = _case(O.PITCH_SHAPE, cuts=[0, 50, 100, 129])
    wide = dict(ldx=c.cin + 32, ldt=c.nt_pad + 8, ldc=c.cout + 4, ldr=c.cout + 8, lde=c.cout + 12, stats_ld=c.cout + 3)
    kw = wide if which == 'all' else {which: wide[which]}
    f = _fwd(c, r, prec, 'pitch ' + which, stats=True, **kw)
    assert f.aux.nbytes == (len(c.multi) + 1) * kw.get('ldx', c.cin) * 4 and len(c.multi) > 0


@pytest.mark.parametrize('prec', O.PRECISIONS)
@pytest.mark.parametrize('epi', list(O.EPILOGUES))
def test_graphconv_fwd_epilogues(epi, prec):
    c, r = _case(O.EPI_SHAPE, epi)
    _fwd(c, r, prec, 'epilogue ' + epi, epi=epi)
    _fwd(c, r, prec, 'epilogue ' + epi, epi=epi, ext=False)


@pytest.mark.parametrize('prec', O.PRECISIONS)
@pytest.mark.parametrize('scalar', ('float4', 'cout3', 'out_off'))
def test_graphconv_fwd_statistics_routes(scalar, prec):
    """wave partials in ws, a ws too small for them (atomics), and the col path in three 128-row chunks, on the float4 and
    the scalar epilogue; labels cut inside the first wave tile, inside the second chunk and on the chunk boundary 256,
    five batch elements of which one is empty"""
    c, r = _case(O.STATS_SHAPE_S if scalar == 'cout3' else O.STATS_SHAPE_V4, cuts=O.STATS_CUTS)
    kw = dict(out_off=4) if scalar == 'out_off' else {}
    part = GM.cdiv(c.n, 32 if c.cout <= 32 else 64) * c.cout * 8
    want = 'atomic' if scalar != 'float4' else None
    f = _fwd(c, r, prec, 'stats partials', stats=True, **kw)
    assert O.stats_route(True, c.n, c.cout, c.Kp, WS_BYTES, scalar == 'float4') == (want or 'partials')
    _fwd(c, r, prec, 'stats small ws', ws_bytes=part - 16, stats=True, **kw)
    assert O.stats_route(True, c.n, c.cout, c.Kp, part - 16, scalar == 'float4') == (want or 'atomic_float4')
    ws3 = O.ws_for_chunk(c.Kp, 128)
    assert [p[1] for p in O.launch_plan(False, c.n, c.cout, c.Kp, ws3, True)] == [128, 128, 44]
    _fwd(c, r, prec, 'stats col chunks', ws_bytes=ws3, stats=True, ext=False, **kw)
    assert O.stats_route(False, c.n, c.cout, c.Kp, ws3, scalar == 'float4') == (want or 'partials')
    # the same chunks without statistics: emb / res walk the chunks alone
    _fwd(c, r, prec, 'col chunks', ws_bytes=ws3, ext=False, **kw)
    assert f.rc == 0


@pytest.mark.parametrize('prec', O.PRECISIONS)
def test_graphconv_fwd_no_multi_segments_and_empty_graph(prec):
    """n_multi = 0 with multi_seg NULL (sizes 0 / 1 / 1): aux is the zero row alone; n_nodes = 0 is OFX_OK, nothing written"""
    c, r = _case(O.NOMULTI_SHAPE, sizes=O.NOMULTI_SIZES)
    assert len(c.multi) == 0
    _fwd(c, r, prec, 'no multi', multi=False, stats=True)
    with _precision(prec):
        f = _fwd_call(c, prec, dict(override=dict(n=0)), True, WS_BYTES)
    assert f.rc == 0 and f.out.untouched() and f.aux.untouched()


def test_graphconv_fwd_refusals():
    """every OFX_EINVAL clause of gather_common and of the entry, one at a time, `out` bit-unchanged"""
    c, r = _case(O.TRIGGER_SHAPE)
    d = _upload(c, c.cin, 0, c.nt_pad)
    ws = _ws().data_ptr()
    bad = [dict(n=-1), dict(cin=0), dict(cout=0), dict(x=None), dict(nbr=None), dict(Wp=None), dict(ldx=c.cin - 1),
           dict(ldc=c.cout - 1), dict(ldr=c.cout - 1), dict(bid=None), dict(lde=c.cout - 1), dict(seg_ptr=None), dict(col=None),
           dict(nt_pad=-32, Kp=c.Kp - c.nt_pad - 32), dict(nt_pad=c.nt_pad + 16, Kp=c.Kp + 16), dict(Kp=c.Kp + 32),
           dict(Kp=c.Kp - 32), dict(tf=None), dict(ldt=c.nt_pad - 4), dict(ldt=c.nt_pad + 2), dict(tf=d.tf + 4),
           dict(stats_ld=c.cout - 1), dict(n_multi=-1), dict(multi=None)]
    with _precision(3):
        ok = _fwd_call(c, 3, dict(stats=True), True, WS_BYTES)
        assert ok.rc == 0 and not ok.out.untouched()
        for ov in bad:
            f = _fwd_call(c, 3, dict(stats=True, override=ov), True, WS_BYTES)
            assert _status(f.rc) == 'invalid argument' and f.out.untouched() and f.aux.untouched(), (ov, _status(f.rc))
        f = _fwd_call(c, 3, dict(override=dict(Wp=_pack(('fwd', id(c)), c.W, c.cin, c.nt, c.Kp, 3) + 4)), True, WS_BYTES)
        assert _status(f.rc) == 'invalid argument' and f.out.untouched()
        f = _fwd_call(c, 3, dict(emb=False, stats=True, override=dict(bid=None)), True, WS_BYTES)      # statistics without labels
        assert _status(f.rc) == 'invalid argument' and f.out.untouched()
        f = _fwd_call(c, 3, dict(override=dict(out=None)), True, WS_BYTES)
        assert _status(f.rc) == 'invalid argument'
        # the col path: no workspace, one off a 16-B boundary, one without room for 128 col rows (ofx.h: 588 * Kp has it)
        for ov in (dict(ws=None, ws_bytes=0), dict(ws=ws + 4), dict(ws_bytes=O.ws_for_chunk(c.Kp, 128) - 128)):
            f = _fwd_call(c, 3, dict(ext=False, override=ov), True, WS_BYTES)
            assert _status(f.rc) == 'invalid argument' and f.out.untouched(), ov
        assert O.ws_for_chunk(c.Kp, 128) <= 588 * c.Kp
        f = _fwd_call(c, 3, dict(ext=False), True, 588 * c.Kp)
        assert f.rc == 0


# ------------------------------------------------------------------------------------------------ ofx_graphconv_bwd_data
def _gather_bwd(entry, prec, what, x, ldx_in, C, n_rows, n_src, nbr, rev_ptr, rev_row, w, ext, multi, Wp, Kp, N, ldo, r, L_,
                simple, use_ext=True, ws_bytes=WS_BYTES, override=None):
    """ofx_graphconv_bwd_data / ofx_gridconv_bwd_data: x = dy [n_src, C] at pitch ldx_in, out = dx [n_rows, N] at pitch ldo"""
    L = _L()
    V = len(multi)
    fast = O.fast_path(C, ldx_in, 0, use_ext, True, 0)
    what = '%s %s %s' % (what, O.PREC_NAME[prec], 'fast' if fast else 'col')
    xbuf, xp = _f32(x, ldx_in)
    tabs = [_i32(t) for t in (nbr.reshape(-1), rev_ptr, rev_row, ext.reshape(-1), multi)]
    wbuf, wp = _f32(torch.from_numpy(np.asarray(w, dtype=np.float32)).reshape(1, -1) if len(w) else torch.zeros(1, 1))

    def call(ws):
        out, aux = _Out(n_rows, N, ldo), _Aux(V, C, ldx_in)
        a = [xp, ldx_in, C] + ([n_rows] if entry == 'ofx_graphconv_bwd_data' else [n_src, n_rows]) + \
            [tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), wp, tabs[3].data_ptr() if use_ext else None,
             tabs[4].data_ptr(), V, aux.ptr, Wp] + ([Kp] if entry == 'ofx_graphconv_bwd_data' else []) + \
            [N, out.ptr, ldo, _ws().data_ptr() if ws else None, ws_bytes if ws else 0]
        if override:
            a[override[0]] = override[1]
        if ws:
            _ws().fill_(0xFF)
        rc = getattr(L.lib(), entry)(*a, L.stream())
        torch.cuda.synchronize()
        return rc, out, aux

    with _precision(prec):
        rc, out, aux = call(False)
        if override:
            assert _status(rc) == 'invalid argument' and out.untouched() and aux.untouched(), what
            rc, out, aux = call(True)
            assert _status(rc) == 'invalid argument' and out.untouched() and aux.untouched(), what
            return
        if fast:
            assert rc == 0, what + ': predicted the branch-free path, ws = NULL gave ' + _status(rc)
        else:
            assert _status(rc) == 'invalid argument' and out.untouched() and aux.untouched(), what + ': predicted the col path'
        rc, out, aux = call(True)
    assert rc == 0, (what, _status(rc))
    plans = O.launch_plan(fast, n_rows, N, Kp, ws_bytes, False)
    name = entry[4:]
    _worst(name, prec, out.check(r, O.bound(prec, r, plans), what))
    if fast:
        rows = aux.rows(what)
        val, mag = O.seg_means(x, rev_ptr, rev_row, w)
        idx = multi.long()
        assert bool((rows[0] == 0).all())
        err = (rows[1:].double() - val[idx]).abs()
        assert bool((err <= O.wsum_err(simple[idx], L_[idx], mag[idx])).all()), what + ': aux sums off'
    else:
        assert aux.untouched()
    _record(name, prec, 'fast' if fast else 'col', O.vec4(N, ldo), max(p_[2].nsplit for p_ in plans) > 1, None)


@pytest.mark.parametrize('prec', O.PRECISIONS)
@pytest.mark.parametrize('shape', O.BWD_SHAPES, ids=lambda s: s[0])
def test_graphconv_bwd_data(shape, prec):
    """weighted reverse CSR whose multi-row segments carry weights other than 1; cout 32 / 64 branch-free, 3 / 24 col;
    ldy > cout and ldx > cin; without the extended table a cout = 32 layer takes the col path; KpT off by 32 is refused"""
    c = O.bwd_case(shape)
    key = ('bwd', shape[0])
    if key not in _REF:
        _REF[key] = O.reference_bwd(c)
    r = _REF[key]
    with _precision(prec):
        Wp = _pack(key, c.WT, c.cout, 0, c.Kp, prec)
    common = (c.dy, c.cout + 4, c.cout, c.n, c.n, c.nbr, c.rev_ptr, c.rev_row, c.w, c.ext, c.multi, Wp, c.Kp, c.cin, c.cin + 4, r,
              c.L, c.simple)
    _gather_bwd('ofx_graphconv_bwd_data', prec, shape[0], *common)
    if c.cout % 32 == 0:
        _gather_bwd('ofx_graphconv_bwd_data', prec, shape[0] + ' no ext', *common, use_ext=False)
    _gather_bwd('ofx_graphconv_bwd_data', prec, shape[0] + ' KpT', *common, override=(13, c.Kp + 32))


# ------------------------------------------------------------------------------------------------ grid convolutions
GRID_ARGS = ('x', 'ldx', 'cin', 'n_in', 'n_out', 'nbr27', 'ext', 'zero', 'Wp', 'cout', 'bias', 'emb', 'lde', 'bid', 'res', 'ldr',
             'out', 'ldc', 'ws', 'ws_bytes')


def _grid_fwd(c, r, prec, what, zero_off=0, nbr27=True, ext=True, expect_einval=False):
    L = _L()
    fast = O.fast_path(c.cin, c.cin + 4, 0, ext, True, zero_off)
    what = '%s %s %s' % (what, O.PREC_NAME[prec], 'fast' if fast else 'col')
    ldx, ldc, ldr, lde = c.cin + 4, c.cout + 4, c.cout + 8, c.cout + 4
    xbuf, xp = _f32(c.x, ldx)
    t1, t2, bid = _i32(c.tab_m1.reshape(-1)), _i32(c.tab.reshape(-1)), _i32(c.bid)
    zbuf, zp = _f32(torch.zeros(1, c.cin), c.cin, zero_off)
    keep = [_f32(c.bias), _f32(c.emb, lde), _f32(c.res, ldr)]

    def call(ws):
        out = _Out(c.n_out, c.cout, ldc)
        a = dict(x=xp, ldx=ldx, cin=c.cin, n_in=c.n_in, n_out=c.n_out, nbr27=t1.data_ptr() if nbr27 else None,
                 ext=t2.data_ptr() if ext else None, zero=zp, cout=c.cout, bias=keep[0][1], emb=keep[1][1], lde=lde,
                 bid=bid.data_ptr(), res=keep[2][1], ldr=ldr, out=out.ptr, ldc=ldc, ws=_ws().data_ptr() if ws else None,
                 ws_bytes=WS_BYTES if ws else 0,
                 Wp=_pack(('grid', c.mode, c.cin, c.cout, id(c)), c.weight, 0, 0, c.Kp, prec, conv3d=(c.cin, c.cout)))
        if ws:
            _ws().fill_(0xFF)
        rc = L.lib().ofx_gridconv_fwd(*[a[k] for k in GRID_ARGS], L.stream())
        torch.cuda.synchronize()
        return rc, out

    with _precision(prec):
        rc, out = call(False)
        if expect_einval:
            assert _status(rc) == 'invalid argument' and out.untouched(), what
            rc, out = call(True)
            assert _status(rc) == 'invalid argument' and out.untouched(), what
            return
        if fast:
            assert rc == 0, what + ': predicted the branch-free path, ws = NULL gave ' + _status(rc)
        else:
            assert _status(rc) == 'invalid argument' and out.untouched(), what + ': predicted the col path'
        rc, out = call(True)
    assert rc == 0, (what, _status(rc))
    plans = O.launch_plan(fast, c.n_out, c.cout, c.Kp, WS_BYTES, False)
    _worst('gridconv_fwd', prec, out.check(r, O.bound(prec, r, plans), what))
    _record('gridconv_fwd', prec, 'fast' if fast else 'col', O.vec4(c.cout, ldc, 0, True, ldr, 0, True, lde),
            max(p_[2].nsplit for p_ in plans) > 1, None)


@pytest.mark.parametrize('prec', O.PRECISIONS)
@pytest.mark.parametrize('width', O.GRID_WIDTHS, ids=lambda w: '%d-%d' % w)
def test_gridconv_fwd_and_bwd_data(width, prec):
    """tap tables of modes 0 / 1 / 2 at depth_out 1 / 2 with B 1 / 3 (8 .. 192 rows, n_in != n_out for modes 1 and 2), bias +
    emb + res; the backward over gridtab_oracle.reverse (multi-row segments under mode 2)"""
    cin, cout = width
    for mode, dd, B in O.GRID_TABLES:
        c = O.grid_case(mode, dd, B, cin, cout)
        key = ('grid', mode, dd, B, cin, cout)
        if key not in _REF:
            _REF[key] = (O.reference_grid(c), O.reference_grid_bwd(c))
        r, rb = _REF[key]
        what = 'grid mode %d depth %d B %d cin %d' % (mode, dd, B, cin)
        _grid_fwd(c, r, prec, what)
        with _precision(prec):
            WpT = _pack(('gridT', mode, cin, cout, id(c)), c.weightT, 0, 0, c.KpT, prec, conv3d=(cout, cin))
        _gather_bwd('ofx_gridconv_bwd_data', prec, what + ' bwd', c.dy, cout + 4, cout, c.n_in, c.n_out, c.rnbr, c.rev_ptr,
                    c.rev_row, c.w, c.rext, c.rmulti, WpT, c.KpT, cin, cin + 4, rb, c.rL, c.rL <= 1)
    if mode == 2:
        assert len(c.rmulti) > 0


@pytest.mark.parametrize('prec', O.PRECISIONS)
def test_gridconv_fwd_path_triggers_and_refusals(prec):
    """zero_row + 4 bytes or no extended table send a cin = 32 layer to the col path; the col path without the -1-padded
    table is OFX_EINVAL"""
    c = O.grid_case(0, 2, 3, 32, 36)
    r = O.reference_grid(c)
    _grid_fwd(c, r, prec, 'grid zero_row + 4', zero_off=4)
    _grid_fwd(c, r, prec, 'grid no ext', ext=False)
    _grid_fwd(c, r, prec, 'grid ext only', nbr27=False)
    _grid_fwd(c, r, prec, 'grid zero_row + 4, no nbr27', zero_off=4, nbr27=False, expect_einval=True)
    c3 = O.grid_case(0, 1, 1, 3, 32)
    _grid_fwd(c3, O.reference_grid(c3), prec, 'grid cin 3, no nbr27', nbr27=False, expect_einval=True)


# ------------------------------------------------------------------------------------------------ ofx_gather_mean
@pytest.mark.parametrize('trig', ('vector', 'cin', 'ldx', 'x_off', 'out_off'))
def test_gather_mean(trig):
    """segments of 0, 1, 2, 255, 256 and 1000 sources; the float4 kernel and each trigger of the scalar one alone"""
    L = _L()
    n = 40
    cin, ldx, x_off, out_off = {'vector': (8, 12, 0, 0), 'cin': (6, 8, 0, 0), 'ldx': (8, 9, 0, 0), 'x_off': (8, 12, 4, 0),
                                'out_off': (8, 12, 0, 4)}[trig]
    seg_ptr, col = GR.hand_csr(5, n, sizes=O.GATHER_MEAN_SIZES)
    assert set(O.GATHER_MEAN_SIZES) <= set(np.diff(seg_ptr).tolist())
    x = GM.operand((n, cin), 6)
    ref, b = O.gather_mean(x, seg_ptr, col)
    xbuf, xp = _f32(x, ldx, x_off)
    sp, cl = _i32(seg_ptr), _i32(col)
    out = _Out(n * 7, cin, cin, out_off)
    L.call('ofx_gather_mean', xp, ldx, cin, n, sp.data_ptr(), cl.data_ptr(), out.ptr, L.stream())
    torch.cuda.synchronize()
    r = dict(ref=ref, S=ref.abs(), written=torch.ones(n * 7, dtype=torch.bool))
    w = out.check(r, b, 'gather_mean ' + trig)
    WORST[('gather_mean', trig)] = w
    COVER[('gather_mean', 'vector' if trig == 'vector' else 'scalar: ' + trig)] = 1
    for a in ((None, ldx, cin, n, sp.data_ptr(), cl.data_ptr(), out.ptr), (xp, ldx, cin, n, None, cl.data_ptr(), out.ptr),
              (xp, ldx, cin, n, sp.data_ptr(), None, out.ptr), (xp, ldx, cin, n, sp.data_ptr(), cl.data_ptr(), None),
              (xp, ldx, 0, n, sp.data_ptr(), cl.data_ptr(), out.ptr), (xp, ldx, cin, -1, sp.data_ptr(), cl.data_ptr(), out.ptr),
              (xp, cin - 1, cin, n, sp.data_ptr(), cl.data_ptr(), out.ptr)):
        assert _status(L.lib().ofx_gather_mean(*a, L.stream())) == 'invalid argument'


# ------------------------------------------------------------------------------------------------ reporting
def test_coverage_table():
    """(runs after the cases of this module) every branch the module was written for was launched, in every precision"""
    print('GCONV_ENTRY coverage: (entry, precision, path, epilogue, split-K, statistics route) -> launches')
    for k in sorted(COVER, key=str):
        print('GCONV_ENTRY   %r: %d' % (k, COVER[k]))
    for prec in O.PRECISIONS:
        for entry in ('graphconv_fwd', 'graphconv_bwd_data', 'gridconv_fwd', 'gridconv_bwd_data'):
            got = {k[2:] for k in COVER if k[:2] == (entry, prec)}
            assert {g[0] for g in got} == {'fast', 'col'}, (entry, prec, got)
        fwd = {k[2:] for k in COVER if k[:2] == ('graphconv_fwd', prec)}
        for path in ('fast', 'col'):
            assert {g[1] for g in fwd if g[0] == path} == {'float4', 'scalar'}, (prec, path)
        assert any(g[2] for g in fwd if g[0] == 'fast'), 'no split-K launch on the branch-free path'
        routes = {(g[0], g[1], g[3]) for g in fwd if g[3]}
        assert routes >= {('fast', 'float4', 'partials'), ('fast', 'float4', 'atomic_float4'), ('fast', 'scalar', 'atomic'),
                          ('col', 'float4', 'partials'), ('col', 'scalar', 'atomic')}, (prec, routes)
        assert {e for p, e in EPI if p == prec} == set(O.EPILOGUES)
    assert {k[1] for k in COVER if k[0] == 'gather_mean'} == {'vector', 'scalar: cin', 'scalar: ldx', 'scalar: x_off',
                                                             'scalar: out_off'}


def test_zz_worst_ratio():
    print('GCONV_ENTRY worst ratio to the bound:', {k: round(v, 4) for k, v in sorted(WORST.items(), key=str)})
    for prec in O.PRECISIONS:
        for entry in ('graphconv_fwd', 'graphconv_bwd_data', 'gridconv_fwd', 'gridconv_bwd_data'):
            assert WORST[(entry, O.PREC_NAME[prec])] <= 1.0
