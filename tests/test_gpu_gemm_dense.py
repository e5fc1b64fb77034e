"""The GEMM core's entry points (csrc/ofx_gemm.hip: ofx_gemm_f32, ofx_gemm_f32_planes, ofx_gather_gemm_f32) one launch at a
time, through octfusion_amd.ops and -- where the wrapper hides an argument -- the C ABI, against the float64 restatement
and the elementwise bounds of tests/gemm_oracle.py, off the shipped shapes: every column tile with ragged rows, columns
and K tails, both weight packings, the bounds-checked flavour, the scalar epilogue, row maps with repeats and skips,
split-K through both reducers with workspaces that force a slice count, pair-plane outputs, the gather-GEMM with zero
rows and a pitched x, and the argument checks.  Every output sits in a sentinel-filled buffer whose pad rows, columns
right of N and rows no out_rows entry names must come back bit-unchanged.  tests/test_gemm_oracle.py shows on the host that
the bounds accept honest arithmetic and reject planted errors, and checks the mirror of the launcher's arithmetic that
names each case's path here (COVER: cases per (flavour, bn, epilogue, reducer, nsplit), printed once)."""
import contextlib

import pytest
import torch

import gemm_oracle as G
from test_gpu_fullwidth import dev, report

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SENT = -12345.678          # outputs: its float32 rounding is compared bit for bit
BIG = 3.0e4                # the columns next to a strided operand: finite, in range, and ruinous if a pitch is wrong
PREC_NAME = {0: 'bf16x3', 1: 'fp32', 2: 'fp16', 3: 'fp16x3'}
COVER = {}                 # (flavour, bn, epilogue, reducer, nsplit, out_planes) -> cases
WORST = {}                 # precision name -> worst |got - ref| / bound seen


@contextlib.contextmanager
def _precision(p):
    from octfusion_amd import ops
    was = ops.get_precision()
    ops.set_precision(PREC_NAME[p])
    try:
        yield
    finally:
        ops.set_precision(was)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _slice_of(t, pitch, col0):
    """Device column slice at column col0 of a BIG-filled [rows, pitch] buffer that holds the host tensor t."""
    buf = torch.full((t.shape[0], pitch), BIG)
    buf[:, col0:col0 + t.shape[1]] = t
    return buf.to(dev())[:, col0:col0 + t.shape[1]]


def _spec(**kw):
    """One launch.  Defaults: contiguous A, bias and res, identity rows, fp32 output with ldc = N rounded up to 4, + 4
    (16-B aligned rows: the float4 epilogue whenever N % 4 == 0), the 96 MB workspace of ops.workspace."""
    sp = dict(kind='dense', prec=3, pack='kn', wkind='unit', a_scale=1.0, bias=True, res=True, lda=None, a_col0=0, ldc=None,
              ldr=None, res_col0=0, a_rows=False, out_rows=False, planes=0, ws='default', seed=0, flavour=None,
              epilogue=None, reducer=None, nsplit=None, table='random', n_src=70)
    sp.update(kw)
    if sp['kind'] == 'gather':
        sp['K'] = sp['cin'] * sp['ntap']
        sp['lda'] = sp['cin'] + 8
        sp['a_col0'] = 4
    M, N, K = sp['M'], sp['N'], sp['K']
    sp['lda'] = sp['lda'] or K + sp['a_col0']
    if sp['ldc'] is None:
        sp['ldc'] = G.cdiv(N, 32) * 32 + 32 if sp['planes'] else G.cdiv(N, 4) * 4 + 4
    sp['ldr'] = sp['ldr'] or N + sp['res_col0']
    ws = sp['ws']
    sp['cell'] = G.cell(sp['prec'], M, N, K, sp['lda'], sp['ldc'], sp['a_col0'] * 4, sp['ldc'] * 4, sp['res'], sp['ldr'],
                        sp['res_col0'] * 4, G.WS_DEFAULT if ws in ('default', None) else ws, ws is not None,
                        sp['kind'] == 'gather')
    for key, got in zip(('flavour', 'bn', 'epilogue', 'reducer', 'nsplit'), sp['cell']):
        assert sp.get(key) in (None, got), 'the case misses the path it was written for: %s = %r, wanted %r (%r)' % (
            key, got, sp[key], kw)
    COVER[sp['cell'] + (sp['planes'],)] = COVER.get(sp['cell'] + (sp['planes'],), 0) + 1
    return sp


def _maps(sp, g):
    """(a_rows, out_rows, rows of A, rows of the destination, m): random source map with repeats whose entries past m
    name other rows than the ones before; destination = a permutation into a taller buffer, every 4th entry negative."""
    M = sp['M']
    n_a, R, a_rows, out_rows, m = M, M, None, None, None
    if sp['a_rows']:
        n_a = M + 37
        a_rows = torch.randint(0, n_a, (M + 9,), generator=g, dtype=torch.int32)
        a_rows[M - 1] = (int(a_rows[0]) + 11) % n_a
        m = M
    if sp['out_rows']:
        R = M + 20
        out_rows = torch.randperm(R, generator=g)[:M].int()
        out_rows[1::4] = -1
        if a_rows is not None:
            out_rows = torch.cat([out_rows, torch.arange(9, dtype=torch.int32)])        # (past m: never read)
    return a_rows, out_rows, n_a, R, m


def _launch(sp, x, pw, bias, res, out, a_rows, out_rows, m, tab=None):
    from octfusion_amd import _lib, ops
    from octfusion_amd._lib import ptr, stream
    M, N, K = sp['M'], sp['N'], sp['K']
    if sp['ws'] == 'default':
        if sp['kind'] == 'gather':
            y = ops.gather_gemm(x, tab, sp['ntap'], pw, M, bias=bias, res=res, out=out, out_rows=out_rows,
                                out_planes=sp['planes'])
        else:
            y = ops.gemm(x, pw, bias=bias, res=res, out=out, a_rows=a_rows, out_rows=out_rows, m=m, out_planes=sp['planes'])
        assert y.data_ptr() == out.data_ptr()
        return None
    assert sp['kind'] == 'dense'
    ws_bytes = sp['ws'] if sp['ws'] is not None else 1 << 20
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev()) if sp['ws'] is not None else None
    _lib.call('ofx_gemm_f32_planes', ptr(x), x.stride(0), ptr(a_rows), M, K, ptr(pw.t), pw.Kp, N, ptr(bias), ptr(res),
              res.stride(0) if res is not None else 0, ptr(out), out.stride(0), ptr(out_rows), ptr(ws), ws_bytes, sp['planes'],
              stream())
    return ws


def _check_planes(buf, R, N, r, bnd, mode, what):
    """Pair-plane output: the 16-bit words of written rows' columns < N are the only ones that may change (a 32-float
    group is one 128-B line [hi x 32 | lo x 32]); read back through ops.planes_merge."""
    from octfusion_amd import ops
    raw = buf.cpu().view(torch.int16)
    sent = torch.full(tuple(buf.shape), SENT).view(torch.int16)
    touched = torch.zeros(raw.shape, dtype=torch.bool)
    n = torch.arange(N)
    hi = (n // 32) * 64 + n % 32
    rows = 1 + torch.nonzero(r['written']).reshape(-1)
    touched[rows[:, None], hi[None, :]] = True
    touched[rows[:, None], hi[None, :] + 32] = True
    assert torch.equal(raw[~touched], sent[~touched]), '%s: a 16-bit word outside the written planes changed' % what
    vals = ops.planes_merge(buf, mode).cpu()[1:1 + R, :N]
    return G.assert_close(vals, r['ref'], r['S'], bnd, what, rows=r['written'])


def _run(sp, A=None):
    """Build the operands of `sp`, launch under its precision, check values, sentinels and (split-K) run-to-run bits."""
    from octfusion_amd import ops
    M, N, K, prec = sp['M'], sp['N'], sp['K'], sp['prec']
    g = torch.Generator().manual_seed(1000 + sp['seed'])
    a_rows, out_rows, n_a, R, m = _maps(sp, g)
    W = G.weight(K, N, 3 * sp['seed'] + 1, sp['wkind'])
    bias = G.operand((N,), 3 * sp['seed'] + 2) if sp['bias'] else None
    res = G.operand((M, N), 3 * sp['seed'] + 3) if sp['res'] else None
    tab = None
    if sp['kind'] == 'gather':
        n_src = M * sp['ntap'] if sp['table'] == 'children' else sp['n_src']
        xh = G.operand((n_src, sp['cin']), 3 * sp['seed'], sp['a_scale'])
        tab = G.gather_table(M, sp['ntap'], n_src, g, sp['table'])
        r = G.gather_gemm(xh, tab, W, bias, res, out_rows, R, full=True)
        if sp['table'] == 'children':                       # Downsample: x.view(-1, 8 C) @ W
            assert torch.equal(r['ref'], G.gemm(xh.reshape(M, -1), W, bias, res, out_rows=out_rows, n_out_rows=R)[0])
    else:
        xh = A if A is not None else G.operand((n_a, K), 3 * sp['seed'], sp['a_scale'])
        r = G.gemm(xh, W, bias, res, a_rows, out_rows, R, m=m, full=True)
    p = G.plan(M, N, K, G.WS_DEFAULT if sp['ws'] in ('default', None) else sp['ws'], sp['ws'] is not None)
    assert (p.bn, p.nsplit) == (sp['cell'][1], sp['cell'][4])
    bnd = G.bound(G.kind_of(sp['cell'][0]), r, G.chain_len(K, p), p.nsplit, sp['planes'])
    what = '%s %s' % (PREC_NAME[prec], {k: v for k, v in sp.items() if k in (
        'kind', 'M', 'N', 'K', 'pack', 'wkind', 'lda', 'a_col0', 'ldc', 'ldr', 'res_col0', 'planes', 'ws', 'cell', 'table')})
    x = _slice_of(xh, sp['lda'], sp['a_col0'])
    assert (x.data_ptr() % 16, x.stride(0)) == ((sp['a_col0'] * 4) % 16, sp['lda'])
    res_d = _slice_of(res, sp['ldr'], sp['res_col0']) if res is not None else None
    d = lambda t: t.to(dev()) if t is not None else None                                  # noqa: E731
    with _precision(prec):
        w_d = (W if sp['pack'] == 'kn' else W.t().contiguous()).to(dev())
        pw = ops.PackedWeight().get(w_d, sp['pack'])
        bufs = []
        for _ in range(2 if p.nsplit > 1 else 1):
            buf = torch.full((R + 2, sp['ldc']), SENT, device=dev())
            out = buf[1:1 + R, :N]
            assert sp['planes'] == 0 or out.data_ptr() % 128 == 0
            keep = _launch(sp, x, pw, d(bias), res_d, out, d(a_rows), d(out_rows), m, d(tab))
            torch.cuda.synchronize()
            del keep
            bufs.append(buf)
    if sp['planes']:
        used = _check_planes(bufs[0], R, N, r, bnd, sp['planes'], what)
    else:
        used = G.check_window(bufs[0].cpu(), 1, N, r, bnd, SENT, what)
    if len(bufs) == 2:
        assert torch.equal(_bits(bufs[0]), _bits(bufs[1])), '%s: two runs of a slice-ordered reduction differ' % what
    WORST[PREC_NAME[prec]] = max(WORST.get(PREC_NAME[prec], 0.0), used)
    return used


def _ids(specs):
    return ['-'.join('%s%s' % (k, sp[k]) for k in ('prec', 'M', 'N', 'K') if k in sp) + '-%d' % i for i, sp in enumerate(specs)]


# ------------------------------------------------------------------------------------------------ a) tiles and tails
TILE = [[_spec(prec=prec, M=M, N=N, K=K, pack=pack, wkind=wkind, bias=i % 2 == 0, res=i % 3 != 1, seed=i,
               flavour=G.flavour(prec, K, K), nsplit=1, epilogue='float4' if N % 4 == 0 else 'scalar')
         for prec in G.PRECISIONS] for i, (M, N, K, pack, wkind) in enumerate(G.TILE_CASES)]


@pytest.mark.parametrize('i', range(len(TILE)), ids=['%d-%d-%d-%s-%s' % c for c in G.TILE_CASES])
def test_tiles_and_tails(i):
    for sp in TILE[i]:
        _run(sp)


KTAIL = [_spec(prec=prec, M=M, N=N, K=K, seed=50 + K, flavour=G.flavour(prec, K, K))
         for prec in (1, 0, 2, 3) for M, N, K in ((129, 33, 36), (127, 130, 100), (5, 5, 36), (257, 64, 100))]


@pytest.mark.parametrize('sp', KTAIL, ids=_ids(KTAIL))
def test_k_tail_rereads_meet_zero_weight_rows(sp):
    """K % 32 != 0 on the branch-free loaders: the k quads past K re-read the LAST FOUR activations (kclamp = K - 4)
    against the zero rows the pack pads the weights with.  Those four are made the largest of the row, so a pad row that
    is not zero, or a clamp that lands elsewhere, is far outside the bound."""
    A = G.operand((sp['M'], sp['K']), 7 * sp['seed'])
    A[:, -4:] = torch.tensor([50.0, -47.0, 44.0, -41.0])
    _run(sp, A)


# ------------------------------------------------------------------------------------------------ b) generic flavour
GENERIC = ([_spec(prec=prec, M=M, N=N, K=K, seed=100 + K, flavour='generic', pack='nk' if K % 2 else 'kn')
            for prec in G.PRECISIONS for K in G.GENERIC_KS
            for M, N in ((129, 33), (5, 130), (257, 32), (130, 64), (7, 132), (33, 5))] +
           [_spec(prec=prec, M=129, N=N, K=36, lda=lda, a_col0=col0, seed=120 + lda, flavour='generic')
            for prec in G.PRECISIONS for N in (32, 65) for lda, col0 in ((37, 0), (41, 4), (40, 1), (44, 3))])


@pytest.mark.parametrize('sp', GENERIC, ids=_ids(GENERIC))
def test_generic_flavour_is_exact_fp32_in_every_precision(sp):
    """K % 4 != 0, lda % 4 != 0, A four bytes off a 16-B boundary: the bounds-checked kernel, held to the exact-fp32 bound
    whatever the precision mode (it reads the fp32 pack)."""
    assert G.kind_of(sp['cell'][0]) == 'exact'
    _run(sp)


# ------------------------------------------------------------------------------------------------ c) scalar epilogue
SCALAR = [_spec(prec=prec, M=129, N=N, K=36, seed=140 + j, epilogue='scalar', flavour=G.flavour(prec, 36, 36), **kw)
          for prec in G.PRECISIONS for N in (32, 64, 132)
          for j, kw in enumerate((dict(ldc=N + 3), dict(ldr=N + 8, res_col0=1), dict(ldr=N + 6, res_col0=4)))]


@pytest.mark.parametrize('sp', SCALAR, ids=_ids(SCALAR))
def test_scalar_epilogue_at_n_multiple_of_4(sp):
    """N % 4 == 0 with ldc % 4 != 0, a res that is not 16-B aligned, ldr % 4 != 0: the float4 epilogue must stand aside."""
    assert sp['N'] % 4 == 0
    _run(sp)


# ------------------------------------------------------------------------------------------------ d) row maps
ROWMAPS = [_spec(prec=prec, M=M, N=N, K=K, a_rows=ar, out_rows=orow, bias=b, res=rs, ldr=N + 12, res_col0=4, seed=160 + j,
                 wkind=('unit', 'decades')[j % 2])
           for prec in G.PRECISIONS
           for j, (M, N, K, ar, orow, b, rs) in enumerate((
               (130, 36, 100, True, False, True, True), (130, 36, 100, False, True, False, True),
               (257, 33, 36, True, True, True, True), (129, 132, 96, True, True, False, False),
               (127, 5, 7, True, True, True, False), (200, 64, 1664, True, True, True, True)))]


@pytest.mark.parametrize('sp', ROWMAPS, ids=_ids(ROWMAPS))
def test_row_maps(sp):
    """a_rows with repeats (longer than m=, its tail naming other rows, and a_rows[M - 1] != M - 1: a clamped tail row that
    ignored the map would read another source), out_rows a permutation into a taller buffer with a quarter skipped, res a
    column slice of a wider tensor (indexed by m, not by the destination row)."""
    _run(sp)


# ------------------------------------------------------------------------------------------------ e) split-K
PER = 130 * 36 * 4
SPLITK = ([_spec(prec=prec, M=M, N=N, K=K, seed=200 + K + N, reducer='float4' if N % 4 == 0 else 'scalar',
                 wkind=('unit', 'small')[K // 256 % 2])
           for prec in G.PRECISIONS for M, N, K in G.SPLITK_CASES] +
          [_spec(prec=prec, M=130, N=36, K=1664, ws=ws, nsplit=ns, seed=230)
           for prec in G.PRECISIONS for ws, ns in ((3 * PER, 3), (2 * PER - 4, 1), (None, 1))] +
          [_spec(prec=prec, M=130, N=35, K=1696, ws=3 * 130 * 35 * 4, nsplit=3, reducer='scalar', seed=231)
           for prec in G.PRECISIONS] +
          [_spec(prec=2, M=130, N=36, K=512, nsplit=4, flavour='bf16x3', seed=232)])


@pytest.mark.parametrize('sp', SPLITK, ids=_ids(SPLITK))
def test_split_k(sp):
    """tiles < 256 and >= 8 k tiles: 2, 4, 13 (= 8 + 4 + 1) and 11 slices (the last one shorter) through the float4 reducer,
    the same through the scalar one (N % 4 != 0); a workspace with room for exactly three slices, for fewer than two (one
    pass), and none.  Each within the bound of ITS slice structure; every split-K launch twice, bit-equal."""
    _run(sp)


def test_split_k_tables_reach_every_reducer_loop():
    ns = sorted({sp['cell'][4] for sp in SPLITK if sp['cell'][3] == 'float4'})
    loops = [G.reducer_loops(n) for n in ns]
    assert all(any(l[i] for l in loops) for i in range(3)), ns
    assert {2, 3, 4, 11, 13} <= set(ns) and {2, 3, 4, 11, 13} <= {sp['cell'][4] for sp in SPLITK if sp['cell'][3] == 'scalar'}
    assert any(sp['cell'][4] == 1 and sp['ws'] != 'default' for sp in SPLITK)


# ------------------------------------------------------------------------------------------------ f) pair planes
PLANES = [_spec(prec=prec, planes=mode, M=M, N=N, K=K, out_rows=orow, bias=b, res=rs, a_rows=orow, seed=260 + j,
                reducer='float4' if K >= 256 else 'none', epilogue='partials' if K >= 256 else 'float4')
          for prec, mode in ((3, 3), (0, 2), (1, 3), (1, 2))
          for j, (M, N, K, orow, b, rs) in enumerate((
              (129, 36, 100, False, True, True), (130, 64, 36, True, False, True), (257, 132, 96, True, True, False),
              (130, 36, 1664, False, True, True), (130, 36, 1696, True, False, False), (130, 260, 512, True, True, True)))]


@pytest.mark.parametrize('sp', PLANES, ids=_ids(PLANES))
def test_pair_plane_outputs(sp):
    """out_planes 3 / 2 from the float4 epilogue and from the float4 split-K reducer (the only reducer that writes
    planes: every split-K case here names it), with and without out_rows, res, bias.  The lines of skipped rows and the
    words of columns >= N stay bit-unchanged."""
    _run(sp)


# ------------------------------------------------------------------------------------------------ g) gather-GEMM
GATHER = [_spec(kind='gather', prec=prec, planes=pl, cin=cin, ntap=ntap, M=n_out, N=G.gather_cout(cin, ntap, n_out) if not pl
                else (32, 64, 132)[j % 3], out_rows=j % 2 == 1, res=j % 3 != 0, bias=j % 4 != 3, ldr=None, seed=300 + j,
                ldc=None, flavour=G.flavour(prec, cin * ntap, cin + 8, gather=True))
          for prec, pl in ((1, 0), (0, 0), (3, 0), (3, 3))
          for j, (cin, ntap, n_out) in enumerate(G.GATHER_CASES)]
DOWNSAMPLE = [_spec(kind='gather', prec=prec, planes=pl, cin=cin, ntap=8, M=n_out, N=2 * cin, table='children', res=False,
                    seed=340 + cin, nsplit=ns)
              for prec, pl in ((1, 0), (0, 0), (3, 0), (3, 3)) for cin, n_out, ns in ((32, 129, 2), (64, 300, 4))]


@pytest.mark.parametrize('sp', GATHER + DOWNSAMPLE, ids=_ids(GATHER + DOWNSAMPLE))
def test_gather_gemm(sp):
    """ops.gather_gemm: x a 16-B aligned column slice (ldx = cin + 8) between BIG columns, table entries in [0, n_src]
    with a fixed share, and whole rows, naming the zero row; 8 x 64 and 27 x 32 / 64 reach split-K; the Downsample table
    against x.view(-1, 8 C) @ W."""
    _run(sp)


# ------------------------------------------------------------------------------------------------ h) refusals
def _refusal_fixture():
    from octfusion_amd import ops
    M, N, K = 16, 32, 32
    t = dict(M=M, N=N, K=K, a=torch.randn(M + 1, K + 8, device=dev()), res=torch.randn(M + 1, N + 8, device=dev()),
             bias=torch.randn(N + 4, device=dev()), out=torch.full((M + 2, 64), SENT, device=dev()),
             ws=torch.empty(1 << 16, dtype=torch.uint8, device=dev()),
             tab=torch.zeros(M * 64, dtype=torch.int32, device=dev()), zero=ops.zero_row(dev()), W=torch.randn(K, N))
    t['pw'] = ops.PackedWeight().get(t['W'].to(dev()), 'kn')
    return t


def _dense_call(t, **kw):
    from octfusion_amd import _lib
    from octfusion_amd._lib import stream
    a = dict(A=t['a'].data_ptr(), lda=t['K'] + 8, a_rows=None, M=t['M'], K=t['K'], Wp=t['pw'].t.data_ptr(), Kp=t['pw'].Kp,
             N=t['N'], bias=None, res=None, ldr=0, out=t['out'].data_ptr() + 64 * 4, ldc=64, out_rows=None,
             ws=t['ws'].data_ptr(), ws_bytes=t['ws'].numel(), mode=0)
    a.update(kw)
    _lib.call('ofx_gemm_f32_planes', a['A'], a['lda'], a['a_rows'], a['M'], a['K'], a['Wp'], a['Kp'], a['N'], a['bias'],
              a['res'], a['ldr'], a['out'], a['ldc'], a['out_rows'], a['ws'], a['ws_bytes'], a['mode'], stream())


def _gather_call(t, **kw):
    from octfusion_amd import _lib
    from octfusion_amd._lib import stream
    a = dict(x=t['a'].data_ptr(), ldx=t['K'] + 8, cin=32, ntap=1, n_src=t['M'], n_out=t['M'], tab=t['tab'].data_ptr(),
             zero=t['zero'].data_ptr(), Wp=t['pw'].t.data_ptr(), Kp=t['pw'].Kp, cout=t['N'], bias=None, res=None, ldr=0,
             out=t['out'].data_ptr() + 64 * 4, ldc=64, out_rows=None, ws=t['ws'].data_ptr(), ws_bytes=t['ws'].numel(), mode=0)
    a.update(kw)
    _lib.call('ofx_gather_gemm_f32', a['x'], a['ldx'], a['cin'], a['ntap'], a['n_src'], a['n_out'], a['tab'], a['zero'],
              a['Wp'], a['Kp'], a['cout'], a['bias'], a['res'], a['ldr'], a['out'], a['ldc'], a['out_rows'], a['ws'],
              a['ws_bytes'], a['mode'], stream())


def test_refusals_and_empty_calls():
    """Every argument check returns OFX_EINVAL before anything is launched: the output stays bit-unchanged.  M == 0 and
    n_out == 0 are accepted and write nothing.  The same calls with valid arguments go through."""
    from octfusion_amd import _lib, ops
    t = _refusal_fixture()
    N, K = t['N'], t['K']
    res, bias, wp = t['res'].data_ptr(), t['bias'].data_ptr(), t['pw'].t.data_ptr()
    untouched = lambda: torch.equal(_bits(t['out']), _bits(torch.full_like(t['out'], SENT)))       # noqa: E731
    dense = [dict(Kp=t['pw'].Kp + 32), dict(Kp=K - 1), dict(lda=K - 1), dict(ldc=N - 1), dict(res=res, ldr=N - 1),
             dict(Wp=wp + 4), dict(mode=1), dict(mode=4),
             # pair planes: whole lines, float4 operands only
             dict(mode=3, N=N - 2), dict(mode=2, ldc=48), dict(mode=3, out=t['out'].data_ptr() + 64 * 4 + 64),
             dict(mode=3, res=res, ldr=N + 2), dict(mode=2, res=res + 4, ldr=N + 8), dict(mode=3, bias=bias + 4),
             dict(mode=3, ws=t['ws'].data_ptr() + 4)]
    gather = [dict(cin=48, Kp=64), dict(cin=16, Kp=32), dict(ldx=K + 6), dict(ntap=65, Kp=65 * 32), dict(n_src=0),
              dict(x=t['a'].data_ptr() + 4), dict(Kp=64), dict(ldc=N - 1), dict(res=res, ldr=N - 1), dict(Wp=wp + 4),
              dict(mode=3, cout=N - 2), dict(mode=3, ldc=48), dict(mode=2, out=t['out'].data_ptr() + 64 * 4 + 64),
              dict(mode=3, res=res, ldr=N + 2)]
    for fn, cases in ((_dense_call, dense), (_gather_call, gather)):
        for kw in cases:
            with pytest.raises(_lib.OfxError, match='invalid argument'):
                fn(t, **kw)
            torch.cuda.synchronize()
            assert untouched(), (fn.__name__, kw)
    _dense_call(t, M=0)
    _dense_call(t, M=0, A=None, out=None)
    _gather_call(t, n_out=0)
    torch.cuda.synchronize()
    assert untouched()
    # valid arguments: the dense call, and the gather call with the identity table, write rows 1 .. M and nothing else
    t['tab'][:t['M']] = torch.arange(t['M'], dtype=torch.int32, device=dev())
    r = G.gemm(t['a'][:t['M'], :K].cpu(), t['W'], t['bias'][:N].cpu(), t['res'][:t['M'], :N].cpu(), full=True)
    bnd = G.bound(G.kind_of(G.flavour(ops.PRECISIONS[ops.get_precision()], K, K + 8)), r, G.pad32(K), 1)
    for fn in (_dense_call, _gather_call):
        t['out'].fill_(SENT)
        fn(t, res=res, ldr=N + 8, bias=bias)
        torch.cuda.synchronize()
        G.check_window(t['out'].cpu(), 1, N, r, bnd, SENT, fn.__name__)


# ------------------------------------------------------------------------------------------------ coverage, worst ratios
def test_coverage_table():
    """Cases per (flavour, bn, epilogue, reducer, nsplit, out_planes), from the launcher mirror the host suite checks
    against its table; no path the shape lists were written for is empty."""
    print('\ncases per (flavour, bn, epilogue, reducer, nsplit, out_planes):')
    for cell in sorted(COVER, key=str):
        print('  %-60s %3d' % (cell, COVER[cell]))
    have = set(COVER)

    def any_cell(**want):
        keys = ('flavour', 'bn', 'epilogue', 'reducer', 'nsplit', 'planes')
        return any(all(c[keys.index(k)] == v for k, v in want.items()) for c in have)
    for flav in ('generic', 'fp32', 'bf16x3', 'fp16x3'):
        for bn in (32, 64, 128):
            for epi in ('float4', 'scalar'):
                assert any_cell(flavour=flav, bn=bn, epilogue=epi), (flav, bn, epi)
    for flav in ('fp32', 'bf16x3', 'fp16x3'):
        for red in ('float4', 'scalar'):
            for ns in (2, 3, 4, 11, 13):
                assert any_cell(flavour=flav, reducer=red, nsplit=ns), (flav, red, ns)
        for planes in (2, 3):
            if (flav, planes) != ('fp16x3', 2) and (flav, planes) != ('bf16x3', 3):
                assert any_cell(flavour=flav, planes=planes, reducer='float4'), (flav, planes)
                assert any_cell(flavour=flav, planes=planes, epilogue='float4'), (flav, planes)
    assert not any(c[5] and c[3] == 'scalar' for c in have)


def test_zz_worst_ratio_per_precision():
    """(runs last in this module) worst |got - ref| / bound over every case above, per precision mode, measured on the GPU."""
    report({'test': 'gemm_dense_worst_ratio_to_bound', 'measured_on_gpu': True, 'worst': WORST})
    assert all(v <= 1.0 for v in WORST.values())
