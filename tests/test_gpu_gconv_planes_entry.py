"""ofx_graphconv_fwd_planes / ofx_graphconv_fwd_planes_cus (csrc/ofx_gemm2.hip, csrc/ofx_gemm3.hip), ofx_pack_weights_planes,
ofx_planes_split / _merge and the three launch knobs one call at a time through the C ABI, with raw framed buffers, so that
no choice of octfusion_amd.ops (contiguous out, ldc = stats_ld = cout, the 96 MB workspace, the full sync buffer, cout % 4
== 0, weights packed from (N, 1) strides) can route a case around the branch it names: the scalar epilogue of all twelve
gconv2_kernel instantiations, pitches wider than the rows, every rung of the persistent launch's fallback ladder, both
values of aux_ready, the per-launch compute-unit count, the pack from three stride layouts, the split, and every
OFX_EINVAL clause.  The reference is the float64 restatement of tests/gconv_planes_oracle.py on hand-made CSRs (empty,
single and multi-source segments); every comparison is elementwise against the DERIVED bound of that module
(tests/test_gconv_planes_oracle.py shows on the host that it admits honest fp32 arithmetic and rejects nine planted
errors).  Every operand sits in a larger allocation with >= 256 bytes of NaN / 0xff on both sides, `out` and `stats`
in sentinel frames that must come back bit-unchanged outside the written window; after every launch the flag words and
the error word of `sync` are zero.  COVER records the branch every launch took, WORST the largest ratio to the bound."""
import contextlib
from types import SimpleNamespace

import pytest
import torch

import gconv_planes_oracle as O
import gn_oracle as GN
from test_gpu_fullwidth import dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SENT = -12345.678
STAT_SENT = 777.25
PAD = 256                          # bytes of frame on each side of an operand
WS_BYTES = 48 << 20
COVER = {}                         # (mode, wm, ni, epilogue, statistics path, launch) -> launches
WORST = {}                         # (mode name, launch) -> worst |got - ref| / bound
ARGS = ('xp', 'ldx', 'cin', 'n', 'seg_ptr', 'col', 'ext', 'multi', 'n_multi', 'aux', 'aux_bytes', 'tfp', 'ldt', 'nt', 'W2',
        'cout', 'bias', 'emb', 'lde', 'bid', 'res', 'ldr', 'out', 'ldc', 'stats', 'stats_ld', 'ws', 'ws_bytes', 'sync',
        'sync_bytes', 'mode', 'aux_ready')
_SHARED = {}
_DEV = {}
_REF = {}


def _L():
    from octfusion_amd import _lib
    return _lib


def _status(rc):
    return _L().lib().ofx_status_string(rc).decode()


def _shared():
    """one workspace and one zeroed sync buffer for the module (one stream)"""
    if not _SHARED:
        _SHARED['ws'] = torch.empty(WS_BYTES, dtype=torch.uint8, device=dev())
        _SHARED['sync'] = torch.zeros(2048, dtype=torch.int32, device=dev())
        _SHARED['cus'] = torch.cuda.get_device_properties(dev()).multi_processor_count
    return _SHARED


@contextlib.contextmanager
def _knobs(tile=0, persistent=1):
    L = _L()
    try:
        L.call('ofx_set_gconv2_tile', tile)
        L.call('ofx_set_gconv_persistent', persistent)
        yield
    finally:
        L.call('ofx_set_gconv2_tile', 0)
        L.call('ofx_set_gconv_persistent', 1)
        L.call('ofx_set_gconv_cus', 0)


def _frame_u8(raw, off=0, fill=0xFF):
    """(device uint8 buffer, byte offset of the data): raw bytes with PAD + off bytes of `fill` in front, PAD behind"""
    flat = raw.contiguous().reshape(-1)
    buf = torch.full((PAD + off + flat.numel() + PAD,), fill, dtype=torch.uint8)
    buf[PAD + off:PAD + off + flat.numel()] = flat
    buf = buf.to(dev())
    assert buf.data_ptr() % 256 == 0
    return buf, PAD + off


def _frame_f32(data, ld, off_bytes=0):
    """[rows, C] fp32 at row pitch ld inside NaN: (device buffer, device pointer of element (0, 0))"""
    rows, C = data.shape
    body = torch.full((rows, ld), float('nan'))
    body[:, :C] = data
    buf, start = _frame_u8(body.view(torch.uint8), off_bytes)
    return buf, buf.data_ptr() + start


def _i32(a, slack=4):
    """int32 device copy with `slack` readable entries behind it (ofx.h: 16 B behind nbr_ext)"""
    t = torch.as_tensor(a).reshape(-1).to(torch.int32)
    return torch.cat([t, torch.zeros(slack, dtype=torch.int32)]).to(dev())


def _case(shape, mode, cuts=None):
    key = (shape[0], mode, cuts is not None)
    if key not in _REF:
        c = O.case(shape, mode, cuts=cuts)
        _REF[key] = (c, O.reference(c))
    return _REF[key]


def _upload(c, ldx=None, x_off=0, ldt=None):
    """The operands of a case that no launch writes, on the device.  ldx / x_off: xp as the byte window [x_off, x_off +
    cin * bpc) of rows of ldx bytes (the rest 0xff: NaN in every format); ldt: type slab pitch."""
    key = (id(c), ldx, x_off, ldt)
    if key in _DEV:
        return _DEV[key]
    L = _L()
    row = c.cin * O.bpc(c.mode)
    ldx = ldx or row
    slab = torch.full((c.n, ldx), 0xFF, dtype=torch.uint8)
    slab[:, x_off:x_off + row] = c.planes
    d = SimpleNamespace(ldx=ldx, x_off=x_off, row=row)
    d.xbuf, xs = _frame_u8(slab)
    d.xp = d.xbuf.data_ptr() + xs + x_off
    d.seg_ptr, d.col = _i32(c.seg_ptr), _i32(c.col)
    d.ext = _i32(c.ext.reshape(-1))                                                     # 16-B aligned, 16 B of slack
    d.ext_un = _i32(torch.cat([torch.zeros(1, dtype=torch.int64), c.ext.reshape(-1)]))  # [1:] is 4 B off a 16-B boundary
    d.multi = _i32(c.multi)
    d.bid = _i32(c.bid)
    d.tfp, d.ldt = None, 0
    if c.ntc:
        d.ldt = ldt or c.tplanes.shape[1]
        tslab = torch.full((c.n, d.ldt), 0xFF, dtype=torch.uint8)
        tslab[:, :c.tplanes.shape[1]] = c.tplanes
        d.tbuf, ts = _frame_u8(tslab)
        d.tfp = d.tbuf.data_ptr() + ts
    nbytes = L.lib().ofx_planes_packed_bytes(c.cin, c.nt, c.cout, c.mode)
    assert nbytes == O.packed_bytes(c.cin, c.nt, c.cout, c.mode)
    d.wbuf, ws = _frame_u8(torch.zeros(nbytes, dtype=torch.uint8))
    d.W2 = d.wbuf.data_ptr() + ws
    Wd = c.W.to(dev())
    L.call('ofx_pack_weights_planes', Wd.data_ptr(), c.cout, 1, c.cin, c.nt, c.cout, c.mode, d.W2, L.stream())
    torch.cuda.synchronize()
    _DEV[key] = d
    return d


def _plan(c, wm, cus=0):
    """(G, words) of ofx_gconv3_plan for the case under tile knob wm"""
    out = torch.zeros(5 + 1024 + 1, dtype=torch.int32)
    G = _L().lib().ofx_gconv3_plan(c.n, c.cout, c.nkt, wm, O.ni_of(c.cout), cus, out.data_ptr(), out.numel())
    return G, out.tolist()


def _launch(c, d, bias=True, emb=True, res=True, stats=True, ldc=None, out_off=0, ldr=None, res_off=0, lde=None,
            bias_off=0, stats_ld=None, ws='full', sync='full', ext_aligned=True, aux_ready=0, aux_bytes=None, n_multi=None,
            multi=True, cus=None, override=None, entry=None):
    """One call.  Offsets in bytes.  Returns rc, the written window of out, whether everything else of the out / stats / aux
    frames is untouched, the stats window and the aux bytes."""
    L, sh = _L(), _shared()
    n, cout, B = c.n, c.cout, c.B
    ldc, ldr, lde, stats_ld = ldc or cout, ldr or cout, lde or cout, stats_ld or cout
    V = len(c.multi) if n_multi is None else n_multi
    obuf, optr = _frame_f32(torch.full((n, ldc), SENT), ldc, out_off)
    host_out0 = obuf.cpu()
    a = dict(xp=d.xp, ldx=d.ldx, cin=c.cin, n=n, seg_ptr=d.seg_ptr.data_ptr(), col=d.col.data_ptr(),
             ext=d.ext.data_ptr() if ext_aligned else d.ext_un.data_ptr() + 4,
             multi=d.multi.data_ptr() if multi else None, n_multi=V, tfp=d.tfp, ldt=d.ldt, nt=c.nt, W2=d.W2, cout=cout,
             lde=lde, ldr=ldr, out=optr, ldc=ldc, stats_ld=stats_ld, mode=c.mode, aux_ready=aux_ready, bias=None, emb=None,
             res=None, stats=None, bid=None)
    keep = [obuf]
    # aux: (V + 1) rows at pitch ldx (+ the window's offset behind the last one), framed; aux_ready = 1: pre-filled
    aux_len = (V + 1) * d.ldx + d.x_off
    araw = torch.full((aux_len,), 0xFF, dtype=torch.uint8)
    if aux_bytes is not None:
        araw = aux_bytes.reshape(-1).clone()
    abuf, astart = _frame_u8(araw)
    a['aux'], a['aux_bytes'] = abuf.data_ptr() + astart + d.x_off, aux_len - d.x_off
    if bias:
        bb, a['bias'] = _frame_f32(c.bias.view(1, cout), cout, bias_off)
        keep.append(bb)
    if emb:
        eb, a['emb'] = _frame_f32(c.emb, lde)
        keep.append(eb)
    if res:
        rb, a['res'] = _frame_f32(c.res, ldr, res_off)
        keep.append(rb)
    if emb or stats:
        a['bid'] = d.bid.data_ptr()
    sbuf = None
    if stats:
        sh0 = torch.full((B + 2, stats_ld, 2), STAT_SENT, dtype=torch.float64)
        sh0[1:B + 1, :cout] = 0.0
        sbuf = sh0.to(dev())
        a['stats'] = sbuf.data_ptr() + stats_ld * 2 * 8
    a['ws'], a['ws_bytes'] = (None, 0) if ws is None else (sh['ws'].data_ptr(), WS_BYTES if ws == 'full' else int(ws))
    a['sync'], a['sync_bytes'] = (None, 0) if sync is None else (sh['sync'].data_ptr(),
                                                                 sh['sync'].numel() * 4 if sync == 'full' else int(sync))
    a.update(override or {})
    args = [a[k] for k in ARGS]
    name = entry or ('ofx_graphconv_fwd_planes' if cus is None else 'ofx_graphconv_fwd_planes_cus')
    if name.endswith('_cus'):
        args.append(0 if cus is None else cus)
    rc = getattr(L.lib(), name)(*args, L.stream())
    torch.cuda.synchronize()
    out = SimpleNamespace(rc=rc, status=_status(rc) if rc else 'ok', keep=keep)
    assert int(sh['sync'].abs().max()) == 0, 'flag words / error word of sync not zero after the launch'
    # out: only the [n, cout] window at pitch ldc may differ from the frame
    host = obuf.cpu()
    start = PAD + out_off
    win = torch.zeros(host.numel(), dtype=torch.bool)
    rows = torch.arange(n)[:, None] * (ldc * 4) + torch.arange(cout * 4)[None, :] + start
    win[rows.reshape(-1)] = True
    out.frame_ok = bool((host == host_out0)[~win].all())
    out.y = host[win].view(torch.float32).view(n, cout)
    out.untouched = bool((host == host_out0).all())
    if stats:
        sc = sbuf.cpu()
        out.stats = sc[1:B + 1, :cout].clone()
        sc[1:B + 1, :cout] = 0.0
        out.stats_frame_ok = torch.equal(sc, sh0)
    ah = abuf.cpu()
    out.aux = ah[astart:astart + aux_len].clone()
    body = torch.zeros(ah.numel(), dtype=torch.bool)
    idx = torch.arange(V + 1)[:, None] * d.ldx + torch.arange(d.row)[None, :] + astart + d.x_off
    body[idx.reshape(-1)] = True
    ref_a = torch.full_like(ah, 0xFF)
    ref_a[astart:astart + aux_len] = araw
    out.aux_frame_ok = bool((ah == ref_a)[~body].all())
    out.aux_rows = ah[idx.reshape(-1)].view(V + 1, d.row)
    return out


def _record(c, wm, epilogue, spath, launch):
    key = (c.mode, wm, O.ni_of(c.cout), epilogue, spath, launch)
    COVER[key] = COVER.get(key, 0) + 1


def _check(c, r, o, launch, pieces=1, what='', stats_path=None, ref=None, S=None):
    """out within the derived bound, frames intact, statistics within theirs"""
    assert o.rc == 0, (what, o.status)
    assert o.frame_ok, what + ': wrote outside the [n, cout] window of out'
    assert o.aux_frame_ok, what + ': wrote outside the aux rows'
    b = O.bound(c.mode, r, c.nkt * O.chunk(c.mode), pieces, c.multi_mask)
    w = O.assert_close(o.y, r['ref'] if ref is None else ref, r['S'] if S is None else S, b, what)
    k = (O.MODE_NAME[c.mode], launch)
    WORST[k] = max(WORST.get(k, 0.0), w)
    if stats_path:
        assert o.stats_frame_ok, what + ': statistics slots beyond cout / outside [0, B) touched'
        s, _ = O.stats_sums(o.y, c.bid, c.B)
        bS, bQ = O.stats_bound(o.y, c.bid, c.B, stats_path)
        dS, dQ = (o.stats[:, :, 0] - s[:, :, 0]).abs(), (o.stats[:, :, 1] - s[:, :, 1]).abs()
        print('GCONV_ENTRY %s: stats worst %.3f / %.3f of the bound' % (what, float((dS / bS.clamp(min=1e-300)).max()),
                                                                      float((dQ / bQ.clamp(min=1e-300)).max())))
        assert bool((dS <= bS).all()) and bool((dQ <= bQ).all()), what + ': fused statistics off'
    return w


# ------------------------------------------------------------------------------------------------ scalar epilogue
@pytest.mark.parametrize('mode', O.MODES)
@pytest.mark.parametrize('shape', O.SCALAR_WIDTHS, ids=lambda s: s[0])
def test_scalar_epilogue_widths(shape, mode):
    """cout 3 (NI = 1; below one float4), 70 and 130 (NI = 2; 130 has a second column tile of 2 columns), bias + emb + res
    + stats, tile knob 2 and 4, `sync` given (the persistent launch must decline) and once without: bit-equal."""
    c, r = _case(shape, mode)
    d = _upload(c)
    assert not O.is_vec4(c.cout, c.cout, ldr=c.cout, lde=c.cout)
    for wm in O.TILES:
        with _knobs(tile=wm):
            o = _launch(c, d)
            _check(c, r, o, 'tile', what='%s mode %d tile %d' % (shape[0], mode, wm), stats_path='scalar')
            _record(c, wm, 'scalar', 'atomic', 'tile')
            o2 = _launch(c, d, sync=None)
            assert o2.rc == 0 and torch.equal(o.y.view(torch.int32), o2.y.view(torch.int32))


@pytest.mark.parametrize('mode', O.MODES)
@pytest.mark.parametrize('trig', O.TRIGGERS)
def test_scalar_epilogue_single_triggers(trig, mode):
    """cout = 128 would take the float4 epilogue; each of these alone sends it to the scalar one"""
    c, r = _case(O.TRIGGER_SHAPE, mode)
    d = _upload(c)
    kw = {'ldc': dict(ldc=c.cout + 1), 'out': dict(out_off=4), 'res': dict(res_off=4), 'ldr': dict(ldr=c.cout + 1),
          'lde': dict(lde=c.cout + 1), 'bias': dict(bias_off=4)}[trig]
    assert O.is_vec4(c.cout, c.cout, ldr=c.cout, lde=c.cout)
    assert not O.is_vec4(c.cout, kw.get('ldc', c.cout), kw.get('out_off', 0), True, kw.get('ldr', c.cout),
                         kw.get('res_off', 0), True, kw.get('lde', c.cout), True, kw.get('bias_off', 0))
    for wm in O.TILES:
        with _knobs(tile=wm):
            o = _launch(c, d, **kw)
            _check(c, r, o, 'tile', what='trigger %s mode %d tile %d' % (trig, mode, wm), stats_path='scalar')
            _record(c, wm, 'scalar', 'atomic', 'tile')


@pytest.mark.parametrize('mode', O.MODES)
def test_scalar_epilogue_batch_labels_inside_one_wave(mode):
    """one, two and three or more batch elements inside a 64-row wave, a boundary on a wave boundary, a 3-row tail"""
    c, r = _case(O.LABEL_SHAPE, mode, cuts=O.LABEL_CUTS)
    d = _upload(c)
    for wm in O.TILES:
        with _knobs(tile=wm):
            o = _launch(c, d)
            _check(c, r, o, 'tile', what='labels mode %d tile %d' % (mode, wm), stats_path='scalar')
            _record(c, wm, 'scalar', 'atomic', 'tile')


# ------------------------------------------------------------------------------------------------ pitches
@pytest.mark.parametrize('mode', O.MODES)
def test_pitches_wider_than_the_rows(mode):
    """xp = the byte window [128, 128 + row) of a 640-byte slab row (channels [32, 96) of 160 in the pair modes), aux at the
    same pitch; ldc, ldr, lde, stats_ld wider than cout; ldt one line wider than the padded type slab (two 32-channel
    tiles for the 63 type rows).  float4 epilogue, two-stage statistics."""
    c, r = _case(O.PITCH_SHAPE, mode)
    d = _upload(c, ldx=640, x_off=128, ldt=c.tplanes.shape[1] + 128)
    cout = c.cout
    kw = dict(ldc=cout + 8, ldr=cout + 4, lde=cout + 12, stats_ld=cout + 3)
    assert O.is_vec4(cout, kw['ldc'], ldr=kw['ldr'], lde=kw['lde'])
    for wm in O.TILES:
        with _knobs(tile=wm):
            assert _plan(c, wm)[0] == 0                     # too few k-step units: the tile launch
            o = _launch(c, d, **kw)
            _check(c, r, o, 'tile', what='pitches mode %d tile %d' % (mode, wm), stats_path='float4')
            _record(c, wm, 'float4', 'partials', 'tile')
            assert bool((o.aux_rows[0] == 0).all())


# ------------------------------------------------------------------------------------------------ fallback ladder
@pytest.mark.parametrize('mode', O.MODES)
def test_fallback_ladder(mode):
    """persistent launch (eligible by ofx_gconv3_plan, a share boundary inside a tile), then every rung that makes
    ofx_launch_gconv3 decline: no workspace, one too small for the statistics partials, one too small for the stream-K
    pieces, no sync, sync too small for the plan, nbr_ext off a 16-B boundary.  The tile-launch rungs are bit-equal to each
    other; the persistent run is another grouping of the same terms."""
    c, r = _case(O.LADDER_SHAPE, mode)
    d = _upload(c)
    part = O.cdiv(c.n, 64) * c.cout * 2 * 4
    used = (part + 255) & ~255
    for wm in O.TILES:
        with _knobs(tile=wm):
            G, words = _plan(c, wm)
            assert G >= 8, 'the case was meant for the persistent launch'
            pieces, cut = O.plan_pieces(words, c.nkt)
            assert cut, 'no share boundary falls inside a tile'
            assert used + G * wm * 64 * 64 * O.ni_of(c.cout) * 4 <= WS_BYTES
            what = 'ladder mode %d tile %d ' % (mode, wm)
            p = _launch(c, d)
            _check(c, r, p, 'persistent', pieces, what + 'persistent', stats_path='float4')
            _record(c, wm, 'float4', 'partials', 'persistent')
            rungs = {'no ws': dict(ws=None), 'ws < partials': dict(ws=part - 16), 'ws < pieces': dict(ws=used + 1024),
                     'no sync': dict(sync=None), 'sync < plan': dict(sync=G * 4), 'nbr_ext unaligned': dict(ext_aligned=False)}
            base = None
            for name, kw in rungs.items():
                o = _launch(c, d, **kw)
                _check(c, r, o, 'tile', 1, what + name, stats_path='float4')
                spath = 'atomic' if name in ('no ws', 'ws < partials') else 'partials'
                _record(c, wm, 'float4', spath, 'rung: ' + name)
                if base is not None:
                    assert torch.equal(o.y.view(torch.int32), base.view(torch.int32)), what + name + ': not bit-equal'
                base = o.y
            bp = O.bound(c.mode, r, c.nkt * O.chunk(c.mode), pieces, c.multi_mask)
            bt = O.bound(c.mode, r, c.nkt * O.chunk(c.mode), 1, c.multi_mask)
            assert bool(((p.y.double() - base.double()).abs() <= bp + bt).all())
            with _knobs(tile=wm, persistent=0):              # the knob itself: the same tile launch
                o = _launch(c, d)
                assert o.rc == 0 and torch.equal(o.y.view(torch.int32), base.view(torch.int32))
                _record(c, wm, 'float4', 'partials', 'rung: persistent off')


# ------------------------------------------------------------------------------------------------ aux_ready
@pytest.mark.parametrize('mode', O.MODES)
@pytest.mark.parametrize('shape', O.AUX_SHAPES, ids=lambda s: s[0])
def test_aux_ready(shape, mode):
    """aux_ready = 0: planes_multi_mean writes the aux rows -- row 0 all zero bytes, the means (segments of 2, 8 and 9
    sources; none at all with multi_seg == NULL) within the mean + re-split bound of the float64 mean of the decoded
    sources; aux_ready = 1 on those bytes: the same output bit for bit."""
    c, r = _case(shape, mode)
    d = _upload(c)
    V = len(c.multi)
    assert (V == 0) == (shape[0] == 'nomulti')
    mean, _ = O.aux(c)
    for wm in O.TILES:
        with _knobs(tile=wm):
            o = _launch(c, d, multi=V > 0)
            _check(c, r, o, 'tile', what='aux_ready 0 %s mode %d tile %d' % (shape[0], mode, wm), stats_path='float4')
            _record(c, wm, 'float4', 'partials', 'aux_ready 0')
            assert o.aux_rows.shape[0] == V + 1 and int(o.aux_rows[0].sum()) == 0
            got = GN.decode(o.aux_rows.contiguous(), c.cin, mode)
            err = (got - mean).abs()
            assert bool((err <= O.aux_err(c)).all()), 'aux rows off: worst %.3e' % float((err - O.aux_err(c)).max())
            if O.pairs(mode) and V:                                # [hi | lo]: the hi halves alone are the rounded means
                hi = GN.decode_hi(o.aux_rows.contiguous(), c.cin, mode)
                rnd = {3: 2.0 ** -11, 2: 2.0 ** -8}[mode]
                assert bool(((hi - mean).abs() <= rnd * mean.abs() + O.aux_err(c) + 2.0 ** -24).all())
            o1 = _launch(c, d, multi=V > 0, aux_ready=1, aux_bytes=o.aux)
            assert o1.rc == 0 and o1.frame_ok
            assert torch.equal(o1.y.view(torch.int32), o.y.view(torch.int32))
            assert torch.equal(o1.aux, o.aux), 'aux_ready = 1 wrote the aux rows'
            _record(c, wm, 'float4', 'partials', 'aux_ready 1')


# ------------------------------------------------------------------------------------------------ _cus
@pytest.mark.parametrize('mode', O.MODES)
def test_cus_entry(mode):
    """cus = 0 is the plain entry bit for bit; 8, 64 and more than the device has (clamped) are planned by ofx_gconv3_plan
    with the same count and stay within the bound; 1..7 and negative counts are refused before any launch"""
    c, r = _case(O.LADDER_SHAPE, mode)
    d = _upload(c)
    dev_cus = _shared()['cus']
    for wm in O.TILES:
        with _knobs(tile=wm):
            plain = _launch(c, d)
            zero = _launch(c, d, cus=0)
            assert plain.rc == 0 and zero.rc == 0 and torch.equal(plain.y.view(torch.int32), zero.y.view(torch.int32))
            for cus in (8, 64, dev_cus + 8):
                G, words = _plan(c, wm, min(cus, dev_cus))
                assert G >= 8
                o = _launch(c, d, cus=cus)
                _check(c, r, o, 'persistent', O.plan_pieces(words, c.nkt)[0], 'cus %d mode %d tile %d' % (cus, mode, wm),
                       stats_path='float4')
                _record(c, wm, 'float4', 'partials', 'cus %s' % ('device + 8' if cus > dev_cus else cus))
            for cus in (-1, 1, 7):
                o = _launch(c, d, cus=cus)
                assert o.status == 'invalid argument' and o.untouched, cus


# ------------------------------------------------------------------------------------------------ pack and split
@pytest.mark.parametrize('mode', O.MODES)
def test_pack_from_three_stride_layouts(mode):
    """(N, 1), the transposed (1, K) and a padded-stride view give the bytes of pack_reference; nt whose 7 nt rows stay in
    one k tile, fill it, cross it; sizes by the header's formula"""
    L = _L()
    cin, cout = 64, 37
    for nt in O.PACK_NTS:
        K = 7 * (cin + O.ntc(nt))
        W = torch.randn(K, cout, generator=torch.Generator().manual_seed(nt + 10 * mode)) * 3.0
        W[5, 2] = O.PROBE_W
        want = O.pack_reference(W, cin, nt, cout, mode)
        assert L.lib().ofx_planes_packed_ktiles(cin, nt, mode) == O.ktiles(cin, nt, mode)
        assert L.lib().ofx_planes_packed_bytes(cin, nt, cout, mode) == want.numel()
        wide = torch.full((K, cout + 3), float('nan'))
        wide[:, :cout] = W
        lay = {'(N, 1)': (W.contiguous().to(dev()), cout, 1), '(1, K)': (W.t().contiguous().to(dev()), 1, K),
               'padded': (wide.to(dev()), cout + 3, 1)}
        for name, (t, sk, sn) in lay.items():
            buf, s = _frame_u8(torch.full((want.numel(),), 0xEE, dtype=torch.uint8), fill=0xEE)
            L.call('ofx_pack_weights_planes', t.data_ptr(), sk, sn, cin, nt, cout, mode, buf.data_ptr() + s, L.stream())
            torch.cuda.synchronize()
            h = buf.cpu()
            got = h[s:s + want.numel()]
            body = want.numel() - O.LINE + 8                  # the lines and the two trailer floats
            assert torch.equal(got[:body], want[:body]), 'pack %s nt %d mode %d' % (name, nt, mode)
            assert bool((h[:s] == 0xEE).all()) and bool((h[s + want.numel():] == 0xEE).all())


@pytest.mark.parametrize('mode', O.MODES)
def test_planes_split_bytes(mode):
    """against gn_oracle.encode byte for byte: Cpad > C zero fill, a wide ldo_bytes with the gap untouched, in place (pair
    modes), n = 0, C < 4 from an unaligned x"""
    L = _L()
    ch, bp = O.chunk(mode), O.bpc(mode)
    g = torch.Generator().manual_seed(mode)

    def run(n, C, Cpad, ldx, x_off_f, ldo, inplace=False):
        x = torch.randn(n, C, generator=g) * 3.0
        xpad = torch.zeros(n, Cpad)
        xpad[:, :C] = x
        want = GN.encode(xpad, mode)
        xbuf, xptr = _frame_f32(x, ldx, x_off_f * 4)
        if inplace:
            assert ldo == ldx * 4 and x_off_f == 0
            obuf, optr, ostart = xbuf, xptr, PAD
            before = xbuf.cpu()
        else:
            obuf, ostart = _frame_u8(torch.full((max(n, 1) * ldo,), 0xEE, dtype=torch.uint8), fill=0xEE)
            optr = obuf.data_ptr() + ostart
            before = obuf.cpu()
        L.call('ofx_planes_split', xptr, ldx, n, C, Cpad, mode, optr, ldo, L.stream())
        torch.cuda.synchronize()
        h = obuf.cpu()
        win = torch.zeros(h.numel(), dtype=torch.bool)
        if n:
            idx = torch.arange(n)[:, None] * ldo + torch.arange(Cpad * bp)[None, :] + ostart
            win[idx.reshape(-1)] = True
            assert torch.equal(h[win].view(n, Cpad * bp), want), (n, C, Cpad, ldo)
        assert bool((h == before)[~win].all()), 'split wrote outside its rows'

    run(130, 45, 2 * ch, 48, 0, 2 * ch * bp)                   # zero fill of [45, Cpad)
    run(130, ch, ch, ch, 0, ch * bp + 64)                      # wide pitch: the gap stays
    run(0, ch, ch, ch, 0, ch * bp)
    run(77, 3, ch, 3, 1, ch * bp)                              # C < 4: scalar loads, x 4 B off, pitch 3
    run(65, 2 * ch, 2 * ch, 2 * ch + 4, 0, 2 * ch * bp)        # pitched x
    if O.pairs(mode):
        run(130, 64, 64, 64, 0, 256, inplace=True)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_of_the_entries():
    """one call per OFX_EINVAL clause, everything else valid, `out` still all sentinel; every clause is tested by the entry
    before its first launch (csrc/ofx_gemm2.hip).  n_nodes = 0 is OFX_OK and writes nothing."""
    c, r = _case(O.PITCH_SHAPE, 3)
    d = _upload(c)
    V = len(c.multi)
    row = c.cin * 4
    ok = _launch(c, d)
    assert ok.rc == 0 and not ok.untouched
    bad = [dict(mode=0), dict(mode=4), dict(n=-1), dict(cin=0), dict(cin=48), dict(cout=0), dict(xp=None),
           dict(seg_ptr=None), dict(col=None), dict(ext=None), dict(aux=None), dict(W2=None), dict(out=None),
           dict(ldx=row - 128), dict(ldx=row + 64), dict(xp=d.xp + 64), dict(W2=d.W2 + 64), dict(ldc=c.cout - 1),
           dict(ldr=c.cout - 1), dict(bid=None, stats=None), dict(lde=c.cout - 1), dict(n_multi=-1), dict(multi=None),
           dict(nt=-1), dict(aux_bytes=(V + 1) * row - 1), dict(tfp=None), dict(ldt=d.ldt + 64), dict(tfp=d.tfp + 64),
           dict(ldt=d.ldt - 128), dict(stats_ld=c.cout - 1)]
    assert d.ldt == 256 and V > 0
    for ov in bad:
        for entry in ('ofx_graphconv_fwd_planes', 'ofx_graphconv_fwd_planes_cus'):
            o = _launch(c, d, override=ov, entry=entry)
            assert o.status == 'invalid argument' and o.untouched, (ov, entry, o.status)
    # aux off a 128-B boundary, statistics without batch ids
    o = _launch(c, d, emb=False, override=dict(bid=None))
    assert o.status == 'invalid argument' and o.untouched
    o = _launch(c, d)
    a_off = _launch(c, d, override=dict(aux=d.xp + 64))
    assert a_off.status == 'invalid argument' and a_off.untouched
    for entry in ('ofx_graphconv_fwd_planes', 'ofx_graphconv_fwd_planes_cus'):
        o = _launch(c, d, override=dict(n=0), entry=entry)
        assert o.rc == 0 and o.untouched and bool((o.aux == 0xFF).all())


def test_refusals_of_pack_split_merge_and_setters():
    L = _L()
    lib = L.lib()
    st = L.stream()
    W = torch.randn(7 * 64, 8).to(dev())
    buf, s = _frame_u8(torch.full((4096 + 7 * 2 * 8 * 128,), 0xEE, dtype=torch.uint8), fill=0xEE)
    o = buf.data_ptr() + s
    before = buf.cpu()

    def einval(rc):
        torch.cuda.synchronize()
        assert _status(rc) == 'invalid argument' and torch.equal(buf.cpu(), before)

    w = W.data_ptr()
    for a in ((None, 8, 1, 64, 0, 8, 3, o), (w, 8, 1, 64, 0, 8, 3, None), (w, 8, 1, 64, 0, 8, 0, o), (w, 8, 1, 64, 0, 8, 4, o),
              (w, 8, 1, 0, 0, 8, 3, o), (w, 8, 1, 48, 0, 8, 3, o), (w, 8, 1, 32, 0, 8, 1, o), (w, 8, 1, 64, -1, 8, 3, o),
              (w, 8, 1, 64, 0, 0, 3, o), (w, 8, 1, 64, 0, 8, 3, o + 8)):
        einval(lib.ofx_pack_weights_planes(*a, st))
    x = torch.randn(16, 64).to(dev())
    xp = x.data_ptr()
    for a in ((xp, 64, 16, 64, 64, 0, o, 256), (xp, 64, 16, 64, 64, 4, o, 256), (xp, 64, -1, 64, 64, 3, o, 256),
              (xp, 64, 16, 0, 64, 3, o, 256), (xp, 64, 16, 64, 32, 3, o, 256), (xp, 64, 16, 40, 48, 3, o, 256),
              (xp, 64, 16, 64, 64, 1, o + 0, 64), (xp, 63, 16, 64, 64, 3, o, 256), (xp, 64, 16, 64, 64, 3, None, 256),
              (xp, 64, 16, 64, 64, 3, o, 240), (xp, 64, 16, 64, 64, 3, o, 264), (xp, 64, 16, 64, 64, 3, o + 8, 256),
              (None, 64, 16, 64, 64, 3, o, 256), (xp, 66, 16, 64, 64, 3, o, 256), (xp + 4, 64, 15, 64, 64, 3, o, 256)):
        einval(lib.ofx_planes_split(*a, st))
    for a in ((o, 256, 4, 64, 0, xp, 64), (o, 256, 4, 64, 4, xp, 64), (o, 256, -1, 64, 3, xp, 64), (o, 256, 4, 0, 3, xp, 64),
              (o, 256, 4, 48, 3, xp, 64), (o, 256, 4, 32, 1, xp, 64), (None, 256, 4, 64, 3, xp, 64),
              (o, 256, 4, 64, 3, None, 64), (o, 256, 4, 64, 3, xp, 63)):
        einval(lib.ofx_planes_merge(*a, st))
    was = lib.ofx_get_precision()
    try:
        for name, vals in (('ofx_set_gconv_persistent', (-1, 3)), ('ofx_set_gconv2_tile', (-1, 1, 3, 8)),
                           ('ofx_set_gconv_cus', (-1, 1, 7)), ('ofx_set_precision', (-1, 4))):
            for v in vals:
                assert _status(getattr(lib, name)(v)) == 'invalid argument', (name, v)
        assert lib.ofx_get_precision() == was
    finally:
        lib.ofx_set_gconv_persistent(1)
        lib.ofx_set_gconv2_tile(0)
        lib.ofx_set_gconv_cus(0)
        lib.ofx_set_precision(was)


# ------------------------------------------------------------------------------------------------ reporting
def test_zz_coverage_and_worst_ratio():
    """(runs last in this module) every branch the module was written for was taken, and the worst ratio to the bound per
    mode and launch shape -- the figures of DESIGN.md"""
    print('GCONV_ENTRY coverage: (mode, wm, ni, epilogue, statistics, launch) -> launches')
    for k in sorted(COVER, key=str):
        print('GCONV_ENTRY   %r: %d' % (k, COVER[k]))
    print('GCONV_ENTRY worst ratio to the bound:', {k: round(v, 4) for k, v in sorted(WORST.items())})
    scalar = {k[:3] for k in COVER if k[3] == 'scalar'}
    assert scalar == {(m, wm, ni) for m in O.MODES for wm in O.TILES for ni in (1, 2)}, sorted(scalar)
    assert {k[4] for k in COVER if k[3] == 'float4'} == {'atomic', 'partials'}
    launches = {k[5] for k in COVER}
    for name in ('persistent', 'rung: no ws', 'rung: ws < partials', 'rung: ws < pieces', 'rung: no sync', 'rung: sync < plan',
                 'rung: nbr_ext unaligned', 'rung: persistent off', 'aux_ready 0', 'aux_ready 1', 'cus 8', 'cus 64',
                 'cus device + 8'):
        assert name in launches, name
    for m in O.MODES:
        assert {k[1] for k in COVER if k[0] == m and k[5] == 'persistent'} == set(O.TILES)
        assert WORST[(O.MODE_NAME[m], 'tile')] <= 1.0 and WORST[(O.MODE_NAME[m], 'persistent')] <= 1.0
