"""The attention entry points (csrc/ofx_dense.hip: ofx_attention, ofx_attention_bwd) one launch at a time, off the shapes the
networks ship with, through octfusion_amd.ops and -- where the wrapper hides an argument (a pitched dqkv, refusals) -- the
C ABI, against the float64 restatement and the elementwise bound of tests/attention_oracle.py: every template width with
channel padding, both staging loops (the scalar one by each of its three triggers), the split-keys kernel on a ragged T,
pitched qkv / out / dout / dqkv, the largest shapes the LDS rule accepts and the first it refuses, and inputs on which a
padded key, a dropped key or a missed max subtraction changes every element.  Every output sits in a sentinel-filled
buffer, operands that are column slices in buffers filled with BIG.  tests/test_attention_oracle.py shows on the host that
the bound accepts honest arithmetic and rejects planted errors, and checks the mirror of the launcher that names each
case's path here (COVER, printed once)."""
import pytest
import torch

import attention_oracle as A
from test_gpu_backward import _within
from test_gpu_fullwidth import dev, errors, report

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SENT = -12345.678          # outputs: its float32 rounding is compared bit for bit (as in tests/test_gpu_gemm_dense.py)
BIG = 3.0e4                # the columns next to a strided operand: finite, in range, and ruinous if a pitch is wrong

COVER = {}                 # (width, split, staging) -> forward cases; ('refused', what) -> refusals
WORST = {}                 # input kind -> worst |got - ref| / bound seen on the GPU

# name -> (qkv column offset, qkv pitch beyond its offset + 3C, out column offset, out pitch beyond C, staging at ch % 4 == 0)
LAYOUTS = {
    'contiguous': (0, 0, 0, 4, 'float4'),
    'qkv_off1': (1, 3, 0, 4, 'base'),          # pitch 3C + 4: a misaligned base with ldq % 4 == 0
    'qkv_pitch3': (0, 3, 0, 4, 'pitch'),       # ldq = 3C + 3
    'qkv_off4': (4, 4, 0, 4, 'float4'),        # ldq = 3C + 8: still 16-byte pieces, a pitch other than 3C
    'out_off3': (0, 0, 3, 4, 'float4'),        # out at column 3 of a buffer C + 7 wide
}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _slice(t, col0, extra):
    """Device column slice at col0 of a BIG-filled [rows, col0 + cols + extra] buffer that holds the host tensor t."""
    buf = torch.full((t.shape[0], col0 + t.shape[1] + extra), BIG)
    buf[:, col0:col0 + t.shape[1]] = t
    return buf.to(dev())[:, col0:col0 + t.shape[1]]


def _window(rows, cols, col0, extra):
    """(buffer, view): a SENT-filled [rows + 2, col0 + cols + extra] device buffer and its [rows, cols] window at (1, col0)."""
    buf = torch.full((rows + 2, col0 + cols + extra), SENT, device=dev())
    return buf, buf[1:1 + rows, col0:col0 + cols]


def _outside_untouched(buf, rows, cols, col0, what):
    raw = _bits(buf.cpu())
    keep = torch.ones(raw.shape, dtype=torch.bool)
    keep[1:1 + rows, col0:col0 + cols] = False
    assert torch.equal(raw[keep], _bits(torch.full_like(buf, SENT).cpu())[keep]), '%s: an element outside the output changed' % what


@pytest.fixture(scope='module')
def refs():
    """(shape, kind) -> (qkv, out64, bound, out32), computed once per case and never changed."""
    cache = {}

    def get(shape, kind):
        if (shape, kind) not in cache:
            B, T, heads, ch = shape
            qkv = A.make(kind, *shape)
            cache[shape, kind] = (qkv,) + A.forward(qkv, B, T, heads) + (A.evaluate(qkv, B, T, heads, torch.float32),)
        return cache[shape, kind]
    return get


def _forward(refs, shape, kind, layout='contiguous', split_on=True):
    from octfusion_amd import _lib, ops
    B, T, heads, ch = shape
    C, rows = heads * ch, B * T
    qoff, qextra, ooff, oextra, staging = LAYOUTS[layout]
    qkv, ref, bound, ref32 = refs(shape, kind)
    x = _slice(qkv, qoff, qextra)
    p = A.path(T, ch, x.stride(0), aligned=x.data_ptr() % 16 == 0, split_on=split_on)
    what = 'attention %r %s %s %s' % (shape, kind, layout, tuple(p))
    assert p.accepted, what
    assert p.staging == (staging if ch % 4 == 0 else 'ch'), 'the case misses the path it was written for: ' + what
    COVER[p[:3]] = COVER.get(p[:3], 0) + 1
    bufs = []
    try:
        _lib.call('ofx_set_attention_split', 1 if split_on else 0)
        for _ in range(2):
            buf, out = _window(rows, C, ooff, oextra)
            assert ops.attention(x, B, T, heads, out=out).data_ptr() == out.data_ptr()
            torch.cuda.synchronize()
            bufs.append(buf)
    finally:
        _lib.call('ofx_set_attention_split', 1)
    got = bufs[0][1:1 + rows, ooff:ooff + C].cpu()
    used = A.ratio(got, ref, bound)
    e, floor = errors(got, ref), errors(ref32, ref)
    report(dict(test='attention_entry_forward', shape=list(shape), kind=kind, layout=layout, split=p.split, width=p.width,
                staging=p.staging, worst_err_over_bound=used, measured_on_gpu=True, out=e, reference_fp32_noise=floor))
    WORST[kind] = max(WORST.get(kind, 0.0), used)
    assert used <= 1.0, (what, used)                                                         # (a)
    _within(e, floor, what)                                                                  # (b)
    _outside_untouched(bufs[0], rows, C, ooff, what)                                         # (c)
    assert torch.equal(_bits(bufs[0]), _bits(bufs[1])), what + ': two launches differ'       # (d)
    return got


FWD = [(s, k) for s in A.FWD_SHAPES for k in A.fwd_kinds(s[1])]


@pytest.mark.parametrize('shape,kind', FWD, ids=['%d-%d-%d-%d-%s' % (s + (k,)) for s, k in FWD])
def test_forward(refs, shape, kind):
    got = _forward(refs, shape, kind)
    if shape[1] == 1:              # one key: softmax = 1, the output is v bit for bit
        assert torch.equal(_bits(got), _bits(A.values(refs(shape, kind)[0], *shape[:3])))


LAID = [(s, l) for s in A.LAYOUT_SHAPES for l in LAYOUTS if l != 'contiguous']


@pytest.mark.parametrize('shape,layout', LAID, ids=['%d-%d-%d-%d-%s' % (s + (l,)) for s, l in LAID])
def test_forward_layouts(refs, shape, layout):
    """qkv one float off a 16-byte boundary, with a pitch that is no multiple of 4, and 16-byte aligned with a pitch
    other than 3C; out a column slice.  Staging differs, the arithmetic does not: bit-equal to the contiguous launch."""
    got = _forward(refs, shape, 'plain', layout)
    assert torch.equal(_bits(got), _bits(_forward(refs, shape, 'plain'))), (shape, layout)


@pytest.mark.parametrize('shape', [s for s in A.FWD_SHAPES if s[1] >= 256], ids=lambda s: '%d-%d-%d-%d' % s)
def test_forward_with_the_split_switched_off(refs, shape):
    """(e) the one-wave-per-32-queries kernel at T >= 256, up to the edge of the LDS envelope."""
    for kind in A.fwd_kinds(shape[1]):
        _forward(refs, shape, kind, split_on=False)


def test_forward_refusals():
    """Every argument check and the LDS rule return OFX_EINVAL before anything is launched: the output stays bit-unchanged.
    The same call with valid arguments goes through."""
    from octfusion_amd import _lib
    from octfusion_amd._lib import stream
    qkv = torch.zeros(545, 3 * 129, device=dev())
    out = torch.full((545, 129), SENT, device=dev())

    def call(T, ch, B=1, heads=1, ldq=None, ldo=None, o=out.data_ptr(), q=qkv.data_ptr()):
        C = heads * ch
        _lib.call('ofx_attention', q, 3 * C if ldq is None else ldq, B, T, heads, ch, o, C if ldo is None else ldo, stream())
    for T, ch in ((545, 32), (289, 64), (129, 128), (545, 1), (289, 33), (129, 65)):
        assert not A.path(T, ch, 3 * ch).accepted and A.path(T - 1, ch, 3 * ch).accepted
    cases = [('lds_545_32', dict(T=545, ch=32)), ('lds_289_64', dict(T=289, ch=64)), ('lds_129_128', dict(T=129, ch=128)),
             ('lds_545_1', dict(T=545, ch=1)), ('lds_289_33', dict(T=289, ch=33)), ('lds_129_65', dict(T=129, ch=65)),
             ('ch_129', dict(T=8, ch=129)), ('ch_0', dict(T=8, ch=0)), ('ldq', dict(T=8, ch=8, heads=2, ldq=47)),
             ('ldo', dict(T=8, ch=8, heads=2, ldo=15)), ('B_0', dict(T=8, ch=8, B=0)), ('T_0', dict(T=0, ch=8)),
             ('heads_0', dict(T=8, ch=8, heads=0)), ('null_out', dict(T=8, ch=8, o=None)), ('null_qkv', dict(T=8, ch=8, q=None))]
    for name, kw in cases:
        with pytest.raises(_lib.OfxError, match='invalid argument'):
            call(**kw)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(torch.full_like(out, SENT))), name
        COVER['refused', name] = 1
    for _ in range(2):                 # a valid call (T = 8: the unsplit kernel) still goes through, twice
        call(T=8, ch=8, heads=2, B=2)
        torch.cuda.synchronize()
        assert torch.equal(out.view(-1)[:16 * 16], torch.zeros(256, device=dev()))          # v = 0
        assert torch.equal(_bits(out.view(-1)[256:]), _bits(torch.full_like(out.view(-1)[256:], SENT)))
        out.fill_(SENT)


# ------------------------------------------------------------------------------------------------ backward
# name -> (qkv column offset, qkv extra pitch, dout column offset, dout extra pitch, staging at ch % 4 == 0)
BWD_LAYOUTS = {
    'contiguous': (0, 0, 0, 0, 'float4'),
    'qkv_off1': (1, 3, 0, 0, 'base'),
    'qkv_pitch3': (0, 3, 0, 0, 'pitch'),
    'qkv_off4': (4, 4, 0, 0, 'float4'),
    'dout_off1': (0, 0, 1, 3, 'base'),
    'dout_pitch3': (0, 0, 0, 3, 'pitch'),
}


@pytest.fixture(scope='module')
def brefs():
    cache = {}

    def get(shape, kind):
        if (shape, kind) not in cache:
            B, T, heads, ch = shape
            qkv = A.make(kind, *shape)
            dout = torch.randn(B * T, heads * ch, generator=torch.Generator().manual_seed(A.seed_of(shape, kind) + 1))
            cache[shape, kind] = (qkv, dout) + A.backward(qkv, dout, B, T, heads)
        return cache[shape, kind]
    return get


def _bwd_abi(x, g, shape, ldd_extra=5):
    """ofx_attention_bwd through the C ABI: dqkv pitched (ldd = 3C + 5) at column 2 of a sentinel buffer, rowstat between
    sentinel guards.  Returns (dqkv on the host, whole buffers for bit comparisons)."""
    from octfusion_amd import _lib
    from octfusion_amd._lib import ptr, stream
    B, T, heads, ch = shape
    C, rows = heads * ch, B * T
    buf, dq = _window(rows, 3 * C, 2, ldd_extra - 2)
    assert dq.stride(0) == 3 * C + ldd_extra
    n = B * heads * T * 3
    rs = torch.full((n + 64,), SENT, device=dev())
    _lib.call('ofx_attention_bwd', ptr(x), x.stride(0), ptr(g), g.stride(0), B, T, heads, ch, rs.data_ptr() + 32 * 4, ptr(dq),
              dq.stride(0), stream())
    torch.cuda.synchronize()
    _outside_untouched(buf, rows, 3 * C, 2, 'attention_bwd %r dqkv' % (shape,))
    guard = torch.cat([rs[:32], rs[32 + n:]])
    assert torch.equal(_bits(guard), _bits(torch.full_like(guard, SENT))), 'attention_bwd %r: rowstat guard changed' % (shape,)
    return buf[1:1 + rows, 2:2 + 3 * C].cpu(), buf


def _backward(brefs, shape, kind, layout='contiguous'):
    from octfusion_amd import ops
    B, T, heads, ch = shape
    qoff, qextra, goff, gextra, staging = BWD_LAYOUTS[layout]
    qkv, dout, g64, g32 = brefs(shape, kind)
    x, g = _slice(qkv, qoff, qextra), _slice(dout, goff, gextra)
    p = A.path(T, ch, x.stride(0), g.stride(0), aligned=(x.data_ptr() | g.data_ptr()) % 16 == 0)
    what = 'attention_bwd %r %s %s %s' % (shape, kind, layout, p.staging)
    assert p.staging == (staging if ch % 4 == 0 else 'ch'), 'the case misses the path it was written for: ' + what
    COVER['bwd', p.staging] = COVER.get(('bwd', p.staging), 0) + 1
    got = ops.attention_backward(x, g, B, T, heads)
    assert torch.equal(_bits(got), _bits(ops.attention_backward(x, g, B, T, heads))), what + ': two launches differ'
    pitched, _ = _bwd_abi(x, g, shape)
    assert torch.equal(_bits(pitched), _bits(got.cpu())), what + ': the pitched dqkv differs from the contiguous one'
    e, floor = errors(got, g64), errors(g32, g64)
    report(dict(test='attention_entry_backward', shape=list(shape), kind=kind, layout=layout, staging=p.staging,
                measured_on_gpu=True, dqkv=e, reference_fp32_noise=floor))
    _within(e, floor, what)
    return got, x, g


BWD = [(s, k) for s in A.BWD_SHAPES for k in A.BWD_KINDS]


@pytest.mark.parametrize('shape,kind', BWD, ids=['%d-%d-%d-%d-%s' % (s + (k,)) for s, k in BWD])
def test_backward(brefs, shape, kind):
    B, T, heads, ch = shape
    got, x, g = _backward(brefs, shape, kind)
    if T == 1:                      # one key: p = 1, dS = 0: dv is dout bit for bit, dq and dk are zero
        d = got.cpu().view(B, heads, 3, ch)
        assert torch.equal(_bits(d[:, :, 2].reshape(B, -1)), _bits(brefs(shape, kind)[1]))
        assert bool((d[:, :, :2] == 0).all())
    if kind == 'plain':             # linear in dout, and scaling by a power of two commutes with every fp32 operation
        for k in (10, 20):
            scaled = _bwd_abi(x, (g * 2.0 ** -k).contiguous(), shape)[0] * 2.0 ** k
            assert torch.equal(_bits(scaled), _bits(got.cpu())), ('gradient scale', shape, k)


BLAID = [(s, l) for s in A.LAYOUT_SHAPES for l in BWD_LAYOUTS if l != 'contiguous']


@pytest.mark.parametrize('shape,layout', BLAID, ids=['%d-%d-%d-%d-%s' % (s + (l,)) for s, l in BLAID])
def test_backward_layouts(brefs, shape, layout):
    _backward(brefs, shape, 'plain', layout)


def test_backward_refusals():
    from octfusion_amd import _lib
    from octfusion_amd._lib import stream
    qkv = torch.zeros(513, 48, device=dev())
    dout = torch.zeros(513, 16, device=dev())
    dq = torch.full((513, 48), SENT, device=dev())
    rs = torch.full((513 * 2 * 3,), SENT, device=dev())

    def call(T=8, ldq=48, ldo=16, ldd=48, B=1, heads=2, ch=8, q=qkv.data_ptr(), g=dout.data_ptr(), r=rs.data_ptr(),
             d=dq.data_ptr()):
        _lib.call('ofx_attention_bwd', q, ldq, g, ldo, B, T, heads, ch, r, d, ldd, stream())
    cases = [('T_513', dict(T=513)), ('T_0', dict(T=0)), ('ldd', dict(ldd=47)), ('ldo', dict(ldo=15)), ('ldq', dict(ldq=47)),
             ('null_rowstat', dict(r=None)), ('null_dqkv', dict(d=None)), ('null_dout', dict(g=None)), ('null_qkv', dict(q=None)),
             ('B_0', dict(B=0)), ('heads_0', dict(heads=0)), ('ch_0', dict(ch=0))]
    for name, kw in cases:
        with pytest.raises(_lib.OfxError, match='invalid argument'):
            call(**kw)
        torch.cuda.synchronize()
        assert torch.equal(_bits(dq), _bits(torch.full_like(dq, SENT))), name
        assert torch.equal(_bits(rs), _bits(torch.full_like(rs, SENT))), name
        COVER['refused', 'bwd_' + name] = 1
    call(T=512)                      # the largest accepted T: dout = 0 gives dqkv = 0 on its 512 rows, nothing below them
    torch.cuda.synchronize()
    assert bool((dq[:512] == 0).all()) and torch.equal(_bits(dq[512:]), _bits(torch.full_like(dq[512:], SENT)))


# ------------------------------------------------------------------------------------------------ coverage, worst ratios
def test_zy_coverage_table():
    """(runs after the cases) forward cases per (width, split, staging) and the refusals, from the launcher mirror the host
    suite checks: no path the shape lists were written for is empty.  Reads the module-level COVER that the tests above
    fill, as tests/test_gpu_gemm_dense.py does: it holds only when the whole file runs in one process in file order, not
    under -k, a distributed run or reordering."""
    print('\nforward cases per (width, split, staging), backward cases per staging, refusals:')
    for cell in sorted(COVER, key=str):
        print('  %-40s %3d' % (cell, COVER[cell]))
    fwd = {c for c in COVER if isinstance(c[0], int)}
    for width in (32, 64, 128):
        assert any(c[0] == width and not c[1] for c in fwd), width
    for width in (32, 64):
        assert any(c[0] == width and c[1] for c in fwd), width
    for staging in ('float4', 'ch', 'pitch', 'base'):
        assert any(c[2] == staging for c in fwd), staging
        assert ('bwd', staging) in COVER, staging
        assert staging == 'ch' or any(c[2] == staging and c[1] for c in fwd), ('split', staging)
    for name in ('lds_545_32', 'lds_289_64', 'lds_129_128', 'ch_129', 'ldq', 'ldo', 'B_0', 'T_0', 'null_out', 'bwd_T_513',
                 'bwd_ldd', 'bwd_ldo', 'bwd_null_rowstat'):
        assert ('refused', name) in COVER, name


def test_zz_worst_ratio_per_input_kind():
    """(runs last in this module) worst |got - out64| / bound over every forward case above, measured on the GPU.  Reads
    the module-level WORST that the forward tests fill: whole file, one process, file order (see the coverage table).
    Measured on an MI355X: plain 0.030, negative 0.032, peaked 0.046, offset 0.083, lastkey 0.010 (fp32 on the CPU: 0.066
    at worst, on offset)."""
    report({'test': 'attention_entry_worst_ratio_to_bound', 'measured_on_gpu': True, 'worst': WORST})
    assert set(WORST) == set(A.KINDS) and all(v <= 1.0 for v in WORST.values())
