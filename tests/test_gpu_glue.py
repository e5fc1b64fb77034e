"""The glue kernels (csrc/ofx_misc.hip, ofx_act) one operator at a time, through octfusion_amd.ops and the C ABI, against
the float64 restatements of tests/glue_oracle.py -- at the shapes include/ofx.h admits rather than the one shape a
shipped config produces: clamped rows and columns, both inner loops of ofx_linear_small, strided and misaligned
operands, maps with skips, the second grid-stride pass (ofx_grid caps a launch at 8192 x 256 = 2 097 152 threads), odd
embedding widths, the alpha clamp.  Every bound is elementwise (glue_oracle.assert_close) with its constant derived
next to the reference it belongs to; tests/test_glue_oracle.py shows on the host that those bounds accept fp32
arithmetic and reject planted errors.  The two embeddings are bounded by the measured float32-vs-float64 difference of
the reference (printed), times four, per value of t."""
import math

import pytest
import torch

import glue_oracle as G
from test_gpu_fullwidth import dev, report

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

GRID_CAP = 8192 * 256
SENT = -12345.678                 # sentinel (its float32 rounding is what gets compared, bit for bit)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _window(rows, cols, pitch, col0, fill=SENT, pad_rows=1):
    """(buffer, view): a [rows, cols] column slice at column col0 of a sentinel-filled [rows + 2 pad, pitch] buffer."""
    buf = torch.full((rows + 2 * pad_rows, pitch), fill, device=dev())
    return buf, buf[pad_rows:pad_rows + rows, col0:col0 + cols]


def _outside_untouched(buf, rows, cols, col0, pad_rows=1):
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[pad_rows:pad_rows + rows, col0:col0 + cols] = False
    return torch.equal(_bits(buf[keep]), _bits(torch.full_like(buf, SENT)[keep]))


# ------------------------------------------------------------------------------------------------ linear_small
# every M instantiation (1, 2, 4, 8, 16) and a clamped row count for MB = 4, 8, 16; K below one float4 step per lane
# (4, 17, 63, 64: idle lanes), not a multiple of 4 (17, 63: the scalar loop), above 256 (260, 1028: a second step);
# N with clamped weight rows (N % 4) and waves that leave before the shuffles (N % 16)
LS_SHAPES = [(1, 4, 1), (2, 17, 3), (3, 63, 16), (4, 64, 17), (5, 260, 30), (8, 1028, 130), (9, 4, 130), (16, 17, 30),
             (1, 1028, 17), (2, 260, 16), (3, 64, 3), (4, 63, 1), (5, 17, 130), (8, 64, 30), (9, 1028, 3), (16, 260, 1),
             (16, 1028, 130), (3, 4, 17)]
LS_ACTS = [(i, o) for i in G.ACTS for o in G.ACTS]


def _ls_check(a, w, bias, res, act_in, act_out, out, what):
    from octfusion_amd import ops
    y = ops.linear_small(a, w, bias=bias, res=res, act_in=act_in, act_out=act_out, out=out)
    M, K = a.shape
    ac, wc = a.cpu(), w.cpu()
    bc = bias.cpu() if bias is not None else None
    rc = res.cpu() if res is not None else None
    ref, S, _ = G.linear_small(ac, wc, bc, rc, act_in, act_out)
    c = G.linear_small_c(ac, K, bc, rc, act_in, act_out)
    used = G.assert_close(y, ref, S, c, what)
    return y, c, used


@pytest.mark.parametrize('i,shape', list(enumerate(LS_SHAPES)), ids=lambda v: str(v).replace(' ', ''))
def test_linear_small_shapes(i, shape):
    M, K, N = shape
    g = _gen(100 + i)
    a = torch.randn(M, K, generator=g).to(dev())
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dev())
    bias = torch.randn(N, generator=g).to(dev()) if i % 2 == 0 else None
    res = torch.randn(M, N, generator=g).to(dev()) if i % 3 != 1 else None
    buf, out = _window(M, N, N + 9, 5)
    y, c, used = _ls_check(a, w, bias, res, None, None, out, 'linear_small %r' % (shape,))
    assert y.data_ptr() == out.data_ptr()
    assert _outside_untouched(buf, M, N, 5), 'wrote outside [0:M, 0:N]'
    print('linear_small', shape, 'c = %.1f, used %.3f of the bound' % (c, used))


@pytest.mark.parametrize('act_in,act_out', LS_ACTS)
@pytest.mark.parametrize('M,K,N', [(5, 260, 17), (3, 17, 30)])
def test_linear_small_activations(M, K, N, act_in, act_out):
    g = _gen(7 * M + K)
    a = (torch.randn(M, K, generator=g) * 1.5).to(dev())
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dev())
    bias = torch.randn(N, generator=g).to(dev())
    res = torch.randn(M, N, generator=g).to(dev()) if act_out != 'silu' else None
    buf, out = _window(M, N, N + 3, 2)
    _ls_check(a, w, bias, res, act_in, act_out, out, 'linear_small %s -> %s' % (act_in, act_out))
    assert _outside_untouched(buf, M, N, 2)


@pytest.mark.parametrize('pitch_a,pitch_w,pitch_o,col_a,vec', [(80, 72, 40, 8, True), (79, 72, 41, 8, False),
                                                              (80, 73, 40, 8, False), (80, 72, 40, 1, False)])
@pytest.mark.parametrize('M', [3, 16])
def test_linear_small_strided_operands(M, pitch_a, pitch_w, pitch_o, col_a, vec):
    """a, w, out and res as column slices of wider buffers: pitches that are multiples of 4 (the float4 loop), pitches
    that are not (the scalar loop at K % 4 == 0), and `a` starting at column 1 (a pointer that is not 16-B aligned)."""
    K, N = 64, 30
    g = _gen(M + pitch_a + col_a)
    abuf = torch.randn(M, pitch_a, generator=g).to(dev())
    wbuf = (torch.randn(N, pitch_w, generator=g) / 8).to(dev())
    rbuf = torch.randn(M, pitch_o + 4, generator=g).to(dev())
    a, w, res = abuf[:, col_a:col_a + K], wbuf[:, 4:4 + K], rbuf[:, 4:4 + N]
    bias = torch.randn(N, generator=g).to(dev())
    is_vec = all(p % 4 == 0 for p in (pitch_a, pitch_w)) and a.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
    assert is_vec == vec                                           # the case is the path it was written for
    buf, out = _window(M, N, pitch_o, 4)
    y, _, _ = _ls_check(a, w, bias, res, 'silu', None, out, 'strided linear_small')
    assert y.data_ptr() == out.data_ptr() and _outside_untouched(buf, M, N, 4)
    # the same operands contiguous: the other loop order, same bound
    _ls_check(a.contiguous(), w.contiguous(), bias, res.contiguous(), 'silu', None, None, 'contiguous linear_small')


def test_linear_small_rejections():
    from octfusion_amd import _lib
    from octfusion_amd._lib import ptr, stream
    K, N = 16, 8
    a = torch.randn(16, K, device=dev())
    w = torch.randn(N, K, device=dev())
    res = torch.randn(16, N, device=dev())
    out = torch.full((17, N), SENT, device=dev())

    def go(M=4, lda=K, r=None, ldr=0):
        _lib.call('ofx_linear_small', ptr(a), lda, M, K, ptr(w), K, N, None, ptr(r), ldr, 0, 0, ptr(out), N, stream())
    for kw in (dict(M=0), dict(M=17), dict(lda=K - 1), dict(r=res, ldr=N - 1)):
        with pytest.raises(_lib.OfxError, match='invalid argument'):
            go(**kw)
        assert torch.equal(_bits(out), _bits(torch.full_like(out, SENT))), kw
    go(r=res, ldr=N)                                               # the same call with valid arguments goes through
    ref = a[:4].double() @ w.double().t() + res[:4].double()
    assert float((out[:4].double() - ref).abs().max()) < 1e-4 and bool((out[4:] == out[16, 0]).all())


# ------------------------------------------------------------------------------------------------ rows_copy
def _maps(n, n_src, n_dst, how, g):
    smap = dmap = None
    if how in ('smap', 'both'):
        smap = torch.randint(0, n_src, (n,), generator=g, dtype=torch.int32)
        smap[::5] = -1
    if how in ('dmap', 'both'):
        dmap = torch.randperm(n_dst, generator=g)[:n].to(torch.int32)          # distinct: no write race
        dmap[2::7] = -1
    return smap, dmap


@pytest.mark.parametrize('how', ['none', 'smap', 'dmap', 'both'])
@pytest.mark.parametrize('C,lds,ldd,col', [(1, 1, 1, 0), (3, 3, 3, 0), (4, 4, 4, 0), (130, 130, 130, 0), (4, 12, 8, 4),
                                           (4, 9, 8, 4), (130, 136, 140, 3), (128, 192, 160, 32)])
def test_rows_copy(how, C, lds, ldd, col):
    """bit-equal to dst[dmap] = src[smap]; C, pitches and column offsets on both sides of the float4 / scalar switch."""
    from octfusion_amd import ops
    n, n_src, n_dst = 300, 340, 360
    g = _gen(C * 1000 + lds + len(how))
    smap, dmap = _maps(n, n_src, n_dst, how, g)
    sbuf = torch.randn(n_src, lds, generator=g)
    col_s = min(col, lds - C)
    dbuf = torch.full((n_dst, ldd), SENT)
    col_d = min(col, ldd - C)
    want, hit = G.rows_copy(sbuf[:, col_s:col_s + C], dbuf[:, col_d:col_d + C], n, smap, dmap)
    full = dbuf.clone()
    full[:, col_d:col_d + C] = want
    sg, dg = sbuf.to(dev()), dbuf.to(dev())
    ops.rows_copy(sg[:, col_s:col_s + C], dg[:, col_d:col_d + C], n, smap=smap.to(dev()) if smap is not None else None,
                  dmap=dmap.to(dev()) if dmap is not None else None)
    assert torch.equal(_bits(dg.cpu()), _bits(full))               # written rows, skipped rows and the columns outside
    assert int(hit.sum()) > 0 and (how == 'none' or int(hit.sum()) < n)
    ops.rows_copy(sg[:, col_s:col_s + C], dg[:, col_d:col_d + C], 0)
    assert torch.equal(_bits(dg.cpu()), _bits(full))               # n = 0 writes nothing


@pytest.mark.parametrize('C', [128, 3])
def test_rows_copy_second_grid_stride_pass(C):
    """n * C / 4 (float4 kernel) and n * C (scalar kernel) just above the 2 097 152 threads of a capped grid."""
    from octfusion_amd import ops
    n = 70000 if C == 128 else 700000
    assert (n * C // 4 if C % 4 == 0 else n * C) > GRID_CAP
    g = _gen(C)
    src = torch.randn(n, C, generator=g).to(dev())
    smap = torch.randperm(n, generator=g).to(torch.int32)
    smap[::1001] = -1
    smap = smap.to(dev())
    dst = torch.full((n, C), SENT, device=dev())
    ops.rows_copy(src, dst, n, smap=smap)
    ok = smap >= 0
    want = torch.full_like(dst, SENT)
    want[ok] = src[smap[ok].long()]
    assert torch.equal(_bits(dst), _bits(want))


@pytest.mark.parametrize('mode', [2, 3])
@pytest.mark.parametrize('C,ldd', [(32, 32), (96, 128), (160, 160), (32, 64)])
def test_rows_copy_planes(mode, C, ldd):
    """the destination rows as hi / lo pair planes: bit-equal to ofx_planes_split (an independent kernel writing the
    same format) of the gathered rows, within the format's rounding of src (fp16 pairs: 2^-22 relative + half an fp16
    subnormal step, 2^-25, where the lo word underflows; bf16 pairs: 2^-17 relative), skipped rows untouched."""
    from octfusion_amd import ops
    n, n_src, n_dst = 200, 230, 260
    g = _gen(mode * 1000 + C + ldd)
    smap, dmap = _maps(n, n_src, n_dst, 'both', g)
    src = torch.randn(n_src, C + 4, generator=g).to(dev())[:, 4:]            # lds = C + 4, 16-B aligned
    dbuf = torch.full((n_dst, ldd), SENT, device=dev())
    dst = dbuf[:, :C]
    before = dbuf.clone()
    ops.rows_copy(src, dst, n, smap=smap.to(dev()), dmap=dmap.to(dev()), planes=mode)
    ok = (smap >= 0) & (dmap >= 0)
    rows_d, rows_s = dmap[ok].long().to(dev()), smap[ok].long().to(dev())
    hit = torch.zeros(n_dst, dtype=torch.bool, device=dev())
    hit[rows_d] = True
    assert 0 < int(hit.sum()) < n
    assert torch.equal(_bits(dbuf[~hit]), _bits(before[~hit])) and torch.equal(_bits(dbuf[:, C:]), _bits(before[:, C:]))
    gathered = src[rows_s].contiguous()
    got = ops.planes_merge(dst, mode)[rows_d]
    assert torch.equal(_bits(got), _bits(ops.planes_merge(ops.planes_split(gathered, mode), mode)))
    err = (got.double() - gathered.double()).abs()
    bound = gathered.double().abs() * (2.0 ** -22 if mode == 3 else 2.0 ** -17) + (2.0 ** -25 if mode == 3 else 0.0)
    assert bool((err <= bound).all()), float((err / bound).max())


# ------------------------------------------------------------------------------------------------ act
@pytest.mark.parametrize('kind', ['none', 'silu', 'gelu'])
@pytest.mark.parametrize('n', [0, 1, 257, GRID_CAP + 3])
def test_act(kind, n):
    """|got - ref| <= c 2^-24 S wherever |ref| > 2^-100, c = glue_oracle.act_c (silu: 10 + 2 |v| sigmoid(-v), five ulp
    for v >= 0; gelu: 12, six ulp) and S = |ref| except for gelu at v < 0 (glue_oracle.act); never NaN; below 2^-100
    the result stays below 2^-99."""
    from octfusion_amd import ops
    g = _gen(n % 1000)
    special = torch.tensor([0.0, -0.0, 100.0, -100.0, 1e4, -1e4])
    x = torch.cat([special, torch.randn(max(n - 6, 0), generator=g) * 3])[:n] if n else torch.zeros(0)
    guard = torch.full((n + 64,), SENT, device=dev())
    y = ops.act(x.to(dev()), kind, out=guard[:n])
    assert bool((guard[n:] == guard[n + 63]).all()) and not bool(torch.isnan(y).any())
    ref, S = G.act(x.double(), None if kind == 'none' else kind)
    c = G.act_c(x, None if kind == 'none' else kind)
    big = ref.abs() > 2.0 ** -100
    yc = y.cpu()
    G.assert_close(yc[big], ref[big], S[big], c[big], 'act ' + kind)
    assert bool((yc[~big].abs() <= 2.0 ** -99).all())
    if kind == 'none':
        assert torch.equal(_bits(yc), _bits(x))


# ------------------------------------------------------------------------------------------------ embeddings
TS = [0.0, 1.0, 0.5, 37.25, 999.0]


def _check_embedding(name, cases, run, ref_fn):
    """cases: list of (label, t, args).  Bound per value of t: four times the largest |float32 - float64| of the host
    reference over every case (the error is the argument's, about |t| times the relative error of the frequency: no
    fixed number is right); at t in {0, 1}, where nothing amplifies, also 1e-6 absolute."""
    margin, got = {}, []
    for label, t, args in cases:
        f64, f32 = ref_fn(t, *args), ref_fn(t, *args, dtype=torch.float32)
        for v in set(t.tolist()):
            rows = t == v
            margin[v] = max(margin.get(v, 0.0), float((f32[rows].double() - f64[rows]).abs().max()))
        got.append((label, t, f64, run(t.to(dev()), *args).cpu()))
    worst = {v: 0.0 for v in margin}
    for label, t, f64, y in got:
        assert y.shape == f64.shape and y.dtype == torch.float32, label
        for i, v in enumerate(t.tolist()):
            worst[v] = max(worst[v], float((y[i].double() - f64[i]).abs().max()))
    report({'test': 'glue_' + name, 'f32_vs_f64_max_per_t': {repr(k): margin[k] for k in sorted(margin)},
            'kernel_vs_f64_max_per_t': {repr(k): worst[k] for k in sorted(worst)}, 'allowed_factor': 4})
    for v in margin:
        assert worst[v] <= 4.0 * margin[v], (name, v, worst[v], margin[v])
        if v in (0.0, 1.0):
            assert worst[v] <= 1e-6, (name, v, worst[v])
    return got


def test_timestep_embedding():
    """layout cos | sin | 0 exactly (the zero column bit-zero), B in {1, 3, 16}, odd dim, dim == 2, fractional t."""
    from octfusion_amd import ops
    cases = []
    for B in (1, 3, 16):
        for dim in (2, 3, 17, 64, 128, 513):
            for mp in (10000.0, 100.0):
                t = torch.tensor([TS[(i + dim + B) % len(TS)] for i in range(B)])
                cases.append(('B%d dim%d mp%g' % (B, dim, mp), t, (dim, mp)))
    got = _check_embedding('timestep_embedding', cases, ops.timestep_embedding, G.timestep_embedding)
    for (label, t, (dim, mp)), (_, _, f64, y) in zip(cases, got):
        half = dim // 2
        if dim % 2:
            assert torch.equal(_bits(y[:, -1]), torch.zeros(len(t), dtype=torch.int32)), label
        zero = t == 0
        assert bool((y[zero][:, :half] == 1).all()) and bool((y[zero][:, half:] == 0).all()), label
        # cos first: at k = 0 the frequency is 1, so column 0 is cos(t) and column half is sin(t)
        assert float((y[:, 0].double() - torch.cos(t.double())).abs().max()) <= 1e-6, label
        assert float((y[:, half].double() - torch.sin(t.double())).abs().max()) <= 1e-6, label


def test_learned_sinusoid():
    """layout t | sin | cos, column 0 bit-equal to t; half in {1, 8, 16}, weights of order 1, t in [0, 1]."""
    from octfusion_amd import ops
    cases = []
    for half in (1, 8, 16):
        for B in (1, 5, 16):
            g = _gen(half * 100 + B)
            w = torch.randn(half, generator=g)
            t = torch.cat([torch.tensor([0.0, 1.0, 0.25, 0.7312, 0.5]), torch.rand(11, generator=g)])[:B]
            cases.append(('half%d B%d' % (half, B), t, (w,)))
    got = _check_embedding('learned_sinusoid', cases, lambda t, w: ops.learned_sinusoid(t, w.to(dev())),
                           G.learned_sinusoid)
    for (label, t, (w,)), (_, _, f64, y) in zip(cases, got):
        half = w.shape[0]
        assert torch.equal(_bits(y[:, 0]), _bits(t)), label
        arg = 2 * math.pi * t.double()[:, None] * w.double()[None]
        assert float((y[:, 1:half + 1].double() - torch.sin(arg)).abs().max()) <= 1e-5, label       # sin before cos
        assert float((y[:, half + 1:].double() - torch.cos(arg)).abs().max()) <= 1e-5, label


# ------------------------------------------------------------------------------------------------ DDIM updates
DDIM_NS = [0, 1, 257, GRID_CAP + 3]


@pytest.mark.parametrize('alpha', [0.9, 1e-3, 1e-9, 0.0])
@pytest.mark.parametrize('n,with_x0', [(0, True), (1, True), (1, False), (257, True), (257, False),
                                       (GRID_CAP + 3, True)])
def test_ddim_eps_update(alpha, n, with_x0):
    """x in place, x0_out = (x - eps sigma) / max(alpha, 1e-8) when given, nothing past n (guard tails); bounds
    glue_oracle.DDIM_EPS_C_X0 = 8 and DDIM_EPS_C_X = 11 roundings on the elementwise term sums."""
    from octfusion_amd import ops
    g = _gen(n % 977 + int(alpha * 10))
    x, eps = torch.randn(n, generator=g), torch.randn(n, generator=g)
    coef = torch.tensor([alpha, 0.43, 0.95, 0.31])
    xn, Sn, x0, S0 = G.ddim_eps(x, eps, coef)
    xb = torch.full((n + 64,), SENT, device=dev())
    xb[:n] = x.to(dev())
    ob = torch.full((n + 64,), SENT, device=dev())
    eg = eps.to(dev())
    xv = xb[:n]
    y = ops.ddim_eps_update(xv, eg, coef.to(dev()), ob[:n] if with_x0 else None)
    assert y is xv                                                 # in place: the values are read from xb below
    G.assert_close(xb[:n], xn, Sn, G.DDIM_EPS_C_X, 'ddim eps x')
    if with_x0:
        G.assert_close(ob[:n], x0, S0, G.DDIM_EPS_C_X0, 'ddim eps x0')
    sent = torch.full((64,), SENT, device=dev())
    assert torch.equal(_bits(xb[n:]), _bits(sent)) and torch.equal(_bits(ob[n if with_x0 else 0:][-64:]), _bits(sent))
    assert torch.equal(eg.cpu(), eps)


@pytest.mark.parametrize('alpha,sd', [(0.9, 0.2), (1e-3, 0.0), (1e-9, 0.2), (0.9, 0.0)])
@pytest.mark.parametrize('n,with_noise', [(0, True), (1, True), (1, False), (257, True), (257, False),
                                          (GRID_CAP + 3, True)])
def test_ddim_x0_update(alpha, sd, n, with_noise):
    """x = alpha_next (x (1 - c) / alpha + c x0) + sd noise in place; noise == NULL is "no noise term" whatever sd is;
    bound glue_oracle.DDIM_X0_C = 10 roundings on the elementwise term sum.  (This update has no clamp: alpha > 0.)"""
    from octfusion_amd import ops
    g = _gen(n % 977 + int(alpha * 10) + 3)
    x, x0, noise = (torch.randn(n, generator=g) for _ in range(3))
    coef = torch.tensor([alpha, 0.37, 0.95, sd])
    ref, S = G.ddim_x0(x, x0, noise if with_noise else None, coef)
    xb = torch.full((n + 64,), SENT, device=dev())
    xb[:n] = x.to(dev())
    ops.ddim_x0_update(xb[:n], x0.to(dev()), noise.to(dev()) if with_noise else None, coef.to(dev()))
    G.assert_close(xb[:n], ref, S, G.DDIM_X0_C, 'ddim x0 x')
    assert torch.equal(_bits(xb[n:]), _bits(torch.full((64,), SENT, device=dev())))


# ------------------------------------------------------------------------------------------------ cat_channels
@pytest.mark.parametrize('zero_copy', [False, True])
def test_cat_channels(zero_copy):
    """the concatenation, and the attached GroupNorm statistics merged: equal to the statistics of the concatenated
    tensor; no statistics unless both sides carry them."""
    from octfusion_amd import ops
    n, Ca, Cb, B = 500, 32, 96, 3
    g = _gen(11)
    full = torch.randn(n, Ca + Cb, generator=g)
    bid = torch.sort(torch.randint(0, B, (n,), generator=g))[0]
    buf = full.to(dev())
    a, b = (buf[:, :Ca], buf[:, Ca:]) if zero_copy else (buf[:, :Ca].contiguous(), buf[:, Ca:].contiguous())
    kw = dict(buf=buf) if zero_copy else {}
    out = ops.cat_channels(a, b, **kw)
    assert ops.get_stats(out) is None and torch.equal(out.cpu(), full)
    if zero_copy:
        assert out.data_ptr() == buf.data_ptr()
    setattr(a, ops.STATS_ATTR, G.group_sums(full[:, :Ca], bid, B).reshape(-1).to(dev()))
    assert ops.get_stats(ops.cat_channels(a, b, **kw)) is None     # one side only
    setattr(b, ops.STATS_ATTR, G.group_sums(full[:, Ca:], bid, B).reshape(-1).to(dev()))
    out = ops.cat_channels(a, b, **kw)
    st = ops.get_stats(out)
    assert st is not None and st.dtype == torch.float64 and st.numel() == B * (Ca + Cb) * 2
    assert torch.equal(st.cpu().view(B, Ca + Cb, 2), G.group_sums(full, bid, B))
    assert torch.equal(out.cpu(), full)
