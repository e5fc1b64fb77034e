"""tests/gemm_oracle.py on the host: honest emulations of the three contraction flavours (an fp32 fma chain; fp16 / bf16 hi +
lo pairs with three products per term and an fp32 accumulator; slice-ordered split-K) stay inside the elementwise bounds
at every shape tests/test_gpu_gemm_dense.py uses, at O(1), 1e-3 activations and 1e-4 / 1e3 / six-decade weights; planted
errors of the kind a tiled kernel makes do not; and the mirror of the launcher's tiling arithmetic matches a hand-written
table.  No GPU, no octfusion_amd."""
import pytest
import torch

import gemm_oracle as G

torch.set_grad_enabled(False)
KINDS = ('exact', 'fp16x3', 'bf16x3')
WORST = {}


def _data(M, N, K, seed, wkind='unit', a_scale=1.0):
    A = G.operand((M, K), seed, a_scale)
    W = G.weight(K, N, seed + 1, wkind)
    bias = G.operand((N,), seed + 2)
    res = G.operand((M, N), seed + 3)
    return A, W, bias, res


def _emu_ok(kind, A, W, bias, res, p, what, out_planes=0):
    K = A.shape[1]
    r = G.gemm(A, W, bias, res, full=True)
    got = G.emulate(kind, A, W, bias, res, p)
    if out_planes:
        got = G.store_planes(got, out_planes)
    b = G.bound(kind, r, G.chain_len(K, p), p.nsplit, out_planes)
    used = G.assert_close(got, r['ref'], r['S'], b, '%s %s' % (kind, what))
    WORST[kind] = max(WORST.get(kind, 0.0), used)
    return used


# ------------------------------------------------------------------------------------------------ emulations pass
@pytest.mark.parametrize('i', range(len(G.TILE_CASES)))
def test_emulations_within_bounds_at_tile_shapes(i):
    M, N, K, _, wkind = G.TILE_CASES[i]
    p = G.plan(M, N, K)
    assert p.nsplit == 1
    for kind in KINDS:
        for a_scale, wk in ((1.0, wkind), (1e-3, 'small'), (1e-3, 'large'), (1.0, 'decades')):
            A, W, bias, res = _data(M, N, K, 10 * i, wk, a_scale)
            _emu_ok(kind, A, W, bias if i % 2 == 0 else None, res if i % 3 != 1 else None, p,
                    'tile case %r x%g %s' % (G.TILE_CASES[i], a_scale, wk))


@pytest.mark.parametrize('K', G.GENERIC_KS)
def test_exact_emulation_at_generic_shapes(K):
    for M, N in ((129, 33), (5, 130)):
        A, W, bias, res = _data(M, N, K, 500 + K)
        assert G.flavour(3, K, K) == 'generic'
        _emu_ok('exact', A, W, bias, res, G.plan(M, N, K), 'generic K = %d' % K)


@pytest.mark.parametrize('M,N,K', G.SPLITK_CASES)
def test_emulations_within_bounds_with_split_k(M, N, K):
    per = M * N * 4
    for ws_bytes in (G.WS_DEFAULT, 3 * per, 2 * per - 4):
        p = G.plan(M, N, K, ws_bytes)
        for kind in KINDS:
            for a_scale, wk in ((1.0, 'unit'), (1e-3, 'small'), (1.0, 'large'))[:3 if ws_bytes == G.WS_DEFAULT else 1]:
                A, W, bias, res = _data(M, N, K, K + N, wk, a_scale)
                _emu_ok(kind, A, W, bias, res, p, 'split-K %r nsplit %d' % ((M, N, K), p.nsplit))
    if N % 4 == 0:
        A, W, bias, res = _data(M, N, K, K + N)
        p = G.plan(M, N, K)
        _emu_ok('fp16x3', A, W, bias, res, p, 'planes 3', out_planes=3)
        _emu_ok('bf16x3', A * 1e-3, W, None, None, p, 'planes 2', out_planes=2)
        _emu_ok('exact', A * 1e-3, W * 1e-4, None, None, p, 'planes 3 tiny', out_planes=3)


@pytest.mark.parametrize('cin,ntap,n_out', G.GATHER_CASES)
def test_emulations_within_bounds_at_gather_shapes(cin, ntap, n_out):
    g = torch.Generator().manual_seed(cin + ntap + n_out)
    n_src, cout = 70, G.gather_cout(cin, ntap, n_out)
    x = G.operand((n_src, cin), 900 + ntap)
    tab = G.gather_table(n_out, ntap, n_src, g)
    W = G.weight(ntap * cin, cout, 901, 'unit')
    rows = G.gather_rows(x, tab).float()
    r = G.gather_gemm(x, tab, W, full=True)
    assert torch.equal(r['ref'], G.gemm(rows, W)[0])
    p = G.plan(n_out, cout, ntap * cin)
    for kind in KINDS:
        got = G.emulate(kind, rows, W, None, None, p)
        b = G.bound(kind, r, G.chain_len(ntap * cin, p), p.nsplit)
        WORST[kind] = max(WORST.get(kind, 0.0), G.assert_close(got, r['ref'], r['S'], b, 'gather %s' % kind))


def test_zz_worst_ratio_of_the_emulations():
    """(runs last in this module) the emulations' worst |got - ref| / bound: a bound an honest implementation sits far
    below is no weaker for it -- a dropped term is off by ~ S / K, see the planted errors -- but one above 1 is wrong."""
    print('worst ratio to the bound, host emulations:', {k: round(v, 4) for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())


# ------------------------------------------------------------------------------------------------ planted errors fail
PM, PN, PK = 130, 36, 100


def _planted(kind, K=PK, wkind='unit', **kw):
    A, W, bias, res = _data(PM, PN, K, 77, wkind)
    p = G.plan(PM, PN, K)
    r = G.gemm(A, W, bias, res, full=True)
    got = G.emulate(kind, A, W, bias, res, p, **kw)
    return got, r, G.bound(kind, r, G.chain_len(K, p), p.nsplit), p


@pytest.mark.parametrize('kind', KINDS)
def test_planted_dropped_k_term_fails(kind):
    got, r, b, _ = _planted(kind)
    G.assert_close(got, r['ref'], r['S'], b)
    got, r, b, _ = _planted(kind, drop_k=[17])
    with pytest.raises(AssertionError, match='worst'):
        G.assert_close(got, r['ref'], r['S'], b)
    # at the largest K of the GPU tests, split and unsplit
    for ws in (True, False):
        A, W, bias, res = _data(PM, PN, 1696, 78)
        p = G.plan(PM, PN, 1696, ws=ws)
        r = G.gemm(A, W, bias, res, full=True)
        b = G.bound(kind, r, G.chain_len(1696, p), p.nsplit)
        G.assert_close(G.emulate(kind, A, W, bias, res, p), r['ref'], r['S'], b)
        with pytest.raises(AssertionError):
            G.assert_close(G.emulate(kind, A, W, bias, res, p, drop_k=[1000]), r['ref'], r['S'], b)


@pytest.mark.parametrize('kind', KINDS)
def test_planted_dropped_k_tile_fails(kind):
    got, r, b, _ = _planted(kind, drop_k=range(32, 64))
    with pytest.raises(AssertionError):
        G.assert_close(got, r['ref'], r['S'], b)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('K,slice_', [(512, 2), (1664, 11), (1696, 10)])
def test_planted_dropped_split_k_slice_fails(kind, K, slice_):
    got, r, b, p = _planted(kind, K=K)
    assert p.nsplit > slice_
    G.assert_close(got, r['ref'], r['S'], b)
    got, r, b, _ = _planted(kind, K=K, drop_slice=slice_)
    with pytest.raises(AssertionError):
        G.assert_close(got, r['ref'], r['S'], b)


@pytest.mark.parametrize('kind', KINDS)
def test_planted_row_from_next_map_entry_fails(kind):
    A, W, bias, res = _data(200, PN, PK, 79)
    a_rows = torch.randint(0, 200, (PM + 1,), generator=torch.Generator().manual_seed(1), dtype=torch.int32)
    p = G.plan(PM, PN, PK)
    r = G.gemm(A, W, bias, res[:PM], a_rows=a_rows[:PM], full=True)
    b = G.bound(kind, r, G.chain_len(PK, p), 1)
    G.assert_close(G.emulate(kind, A[a_rows[:PM].long()], W, bias, res, p), r['ref'], r['S'], b)
    with pytest.raises(AssertionError):
        G.assert_close(G.emulate(kind, A[a_rows[1:].long()], W, bias, res, p), r['ref'], r['S'], b)
    # only the LAST row wrong (a tile's clamped tail taking another source than row M - 1)
    rows = A[a_rows[:PM].long()].clone()
    rows[-1] = A[a_rows[PM].long()]
    with pytest.raises(AssertionError, match=r'\(m, n\) = \(%d,' % (PM - 1)):
        G.assert_close(G.emulate(kind, rows, W, bias, res, p), r['ref'], r['S'], b)


def test_planted_skipped_row_written_anyway_fails():
    A, W, bias, res = _data(PM, PN, PK, 80)
    out_rows = torch.randperm(PM + 20, generator=torch.Generator().manual_seed(2))[:PM].int()
    out_rows[::4] = -1
    r = G.gemm(A, W, bias, res, out_rows=out_rows, n_out_rows=PM + 20, full=True)
    assert int(r['written'].sum()) == int((out_rows >= 0).sum()) < PM
    p = G.plan(PM, PN, PK)
    val = G.emulate('exact', A, W, bias, res, p)
    b = G.bound('exact', r, G.chain_len(PK, p), 1)
    sent = -12345.678

    def buffer(skip_to=None):
        buf = torch.full((PM + 22, PN + 4), sent)
        for m in range(PM):
            o = int(out_rows[m])
            if o < 0 and skip_to is None:
                continue
            buf[1 + (o if o >= 0 else skip_to), :PN] = val[m]
        return buf
    G.check_window(buffer(), 1, PN, r, b, sent)
    free = int(torch.nonzero(~r['written'])[0])
    for where in (-1, free):           # the store that ignores the sign lands one row before the buffer; or on a free row
        with pytest.raises(AssertionError, match='untouched'):
            G.check_window(buffer(where), 1, PN, r, b, sent)
    spill = buffer()
    spill[1 + int(out_rows[1]), PN] = val[1, 0]                       # one float past N
    with pytest.raises(AssertionError, match='untouched'):
        G.check_window(spill, 1, PN, r, b, sent)


@pytest.mark.parametrize('kind', KINDS)
def test_planted_residual_read_with_pitch_n_fails(kind):
    A, W, bias, _ = _data(PM, PN, PK, 81)
    ldr = PN + 12
    rbuf = G.operand((PM, ldr), 82)
    res = rbuf[:, 4:4 + PN]
    wrong = rbuf.reshape(-1)[4:4 + PM * PN].reshape(PM, PN)           # the same base, pitch N
    p = G.plan(PM, PN, PK)
    r = G.gemm(A, W, bias, res, full=True)
    b = G.bound(kind, r, G.chain_len(PK, p), 1)
    G.assert_close(G.emulate(kind, A, W, bias, res, p), r['ref'], r['S'], b)
    with pytest.raises(AssertionError):
        G.assert_close(G.emulate(kind, A, W, bias, wrong, p), r['ref'], r['S'], b)


def test_planted_dropped_lo_half_fails_fp16x3_passes_bf16x3():
    """One activation entering with its fp16 hi half only (11 bits instead of 22): off by |a_lo w| <= 2^-11 |a w|, which
    the fp16x3 bound (~2^-22 per term) must reject and the bf16x3 bound (3 * 2^-16 per term, 2^-16 S >> 2^-11 |a w| for a
    term that is ~ 1 / K of S) must accept -- the two bounds are not interchangeable."""
    K = 36
    A, W, bias, res = _data(PM, PN, K, 83, 'plain')
    p = G.plan(PM, PN, K)
    r = G.gemm(A, W, bias, res, full=True)
    ah = A.half().float()
    al = (A - ah).abs()
    k0 = 9
    m0 = int((al[:, k0] / A[:, k0].abs().clamp(min=1e-30)).argmax())   # the row whose lo half matters most
    got = G.emulate('fp16x3', A, W, bias, res, p, drop_lo=(m0, k0))
    with pytest.raises(AssertionError, match=r'\(m, n\) = \(%d,' % m0):
        G.assert_close(got, r['ref'], r['S'], G.bound('fp16x3', r, G.chain_len(K, p), 1))
    G.assert_close(got, r['ref'], r['S'], G.bound('bf16x3', r, G.chain_len(K, p), 1))


@pytest.mark.parametrize('wkind', ['unit', 'small', 'large'])
def test_planted_weight_scale_not_undone_fails(wkind):
    got, r, b, _ = _planted('fp16x3', wkind=wkind, keep_scale=True)
    assert G.weight_scale(r['wmax']) != 1.0
    with pytest.raises(AssertionError):
        G.assert_close(got, r['ref'], r['S'], b)


def test_bound_of_an_element_is_its_own():
    """Scaling one output row's operands by 1e6 must leave every other row's bound unchanged (no relative-to-max)."""
    A, W, bias, res = _data(8, 12, 36, 84)
    p = G.plan(8, 12, 36)
    for kind in KINDS:
        b0 = G.bound(kind, G.gemm(A, W, bias, res, full=True), 64, 1)
        A2, res2 = A.clone(), res.clone()
        A2[3] *= 1e3
        res2[3] *= 1e6
        b1 = G.bound(kind, G.gemm(A2, W, bias, res2, full=True), 64, 1)
        keep = torch.arange(8) != 3
        assert torch.equal(b0[keep], b1[keep]) and bool((b1[3] > b0[3]).all())


def test_weight_scale_window():
    for wmax in (1e-4, 0.37, 1.0, 50.0, 1e3, 2.0 ** 14, 65504.0):
        s = G.weight_scale(wmax)
        assert 2.0 ** 14 <= float(torch.tensor(wmax, dtype=torch.float32)) * s < 2.0 ** 15
    assert G.weight_scale(0.0) == 1.0


# ------------------------------------------------------------------------------------------------ launcher decisions
PER = 130 * 36 * 4
PLAN_TABLE = [
    # M, N, K, ws_bytes, ws        bn  ntm ntn nsplit kt_per_split
    ((1, 1, 4, G.WS_DEFAULT, True), (32, 1, 1, 1, 1)),
    ((257, 32, 100, G.WS_DEFAULT, True), (32, 3, 1, 1, 4)),
    ((129, 33, 96, G.WS_DEFAULT, True), (64, 2, 1, 1, 3)),
    ((128, 64, 36, G.WS_DEFAULT, True), (64, 1, 1, 1, 2)),
    ((257, 65, 4, G.WS_DEFAULT, True), (128, 3, 1, 1, 1)),
    ((257, 260, 100, G.WS_DEFAULT, True), (128, 3, 3, 1, 4)),
    ((130, 36, 224, G.WS_DEFAULT, True), (64, 2, 1, 1, 7)),           # 7 k tiles: below the split-K threshold
    ((130, 36, 256, G.WS_DEFAULT, True), (64, 2, 1, 2, 4)),
    ((130, 36, 512, G.WS_DEFAULT, True), (64, 2, 1, 4, 4)),
    ((130, 36, 1664, G.WS_DEFAULT, True), (64, 2, 1, 13, 4)),         # 13 = 8 + 4 + 1
    ((130, 36, 1696, G.WS_DEFAULT, True), (64, 2, 1, 11, 5)),         # 53 k tiles: ten slices of 5 and one of 3
    ((130, 35, 1696, G.WS_DEFAULT, True), (64, 2, 1, 11, 5)),
    ((130, 36, 1664, 3 * PER, True), (64, 2, 1, 3, 18)),              # room for exactly three slices: 18 + 18 + 16
    ((130, 36, 1664, 3 * PER - 1, True), (64, 2, 1, 2, 26)),
    ((130, 36, 1664, 2 * PER - 4, True), (64, 2, 1, 1, 52)),          # fewer than two: a single pass
    ((130, 36, 1664, 0, True), (64, 2, 1, 1, 52)),
    ((130, 36, 1664, G.WS_DEFAULT, False), (64, 2, 1, 1, 52)),        # ws = NULL
    ((300, 64, 512, G.WS_DEFAULT, True), (64, 3, 1, 4, 4)),
    ((300, 132, 1728, G.WS_DEFAULT, True), (128, 3, 2, 11, 5)),
    ((1, 1, 8192, G.WS_DEFAULT, True), (32, 1, 1, 64, 4)),            # the 64-slice cap
    ((12800, 32, 2048, G.WS_DEFAULT, True), (32, 100, 1, 6, 11)),     # 512 / 100 tiles -> 6 slices: five of 11, one of 9
    ((32768, 128, 512, G.WS_DEFAULT, True), (128, 256, 1, 1, 16)),    # 256 tiles: no split-K
]


@pytest.mark.parametrize('args,want', PLAN_TABLE, ids=lambda v: str(v).replace(' ', ''))
def test_launcher_plan_table(args, want):
    assert tuple(G.plan(*args)) == want


def test_launcher_flavour_epilogue_and_reducer():
    assert G.flavour(1, 36, 36) == 'fp32' and G.flavour(3, 36, 36) == 'fp16x3'
    assert G.flavour(0, 36, 36) == G.flavour(2, 36, 36) == 'bf16x3'
    for K, lda, off in ((1, 4, 0), (3, 4, 0), (7, 8, 0), (30, 32, 0), (36, 37, 0), (36, 40, 4), (36, 40, 8)):
        assert G.flavour(3, K, lda, off) == 'generic'
    assert G.flavour(3, 36, 40, 16) == 'fp16x3' and G.flavour(3, 32, 33, gather=True) == 'fp16x3'
    assert G.kind_of('generic') == G.kind_of('fp32') == 'exact' and G.kind_of('bf16x3') == 'bf16x3'
    assert G.vec4(64, 68) and not G.vec4(65, 68) and not G.vec4(64, 67) and not G.vec4(64, 68, out_off_bytes=4)
    assert G.vec4(64, 68, res=True, ldr=72) and not G.vec4(64, 68, res=True, ldr=70)
    assert not G.vec4(64, 68, res=True, ldr=72, res_off_bytes=4) and not G.vec4(64, 68, bias_off_bytes=8)
    assert G.reducer_loops(13) == (1, 1, 1) and G.reducer_loops(11) == (1, 0, 3) and G.reducer_loops(4) == (0, 1, 0)
    assert G.reducer_loops(2) == (0, 0, 2) and G.reducer_loops(3) == (0, 0, 3)
    assert G.cell(3, 130, 36, 1664, 1664, 64) == ('fp16x3', 64, 'partials', 'float4', 13)
    assert G.cell(1, 130, 35, 256, 256, 36) == ('fp32', 64, 'partials', 'scalar', 2)
    assert G.cell(0, 129, 260, 7, 7, 260) == ('generic', 128, 'float4', 'none', 1)
    assert G.cell(0, 129, 64, 36, 36, 67) == ('bf16x3', 64, 'scalar', 'none', 1)
    # the split-K shapes run all three loops of the float4 reducer, and one has a shorter last slice
    loops = [G.reducer_loops(G.plan(M, N, K).nsplit) for M, N, K in G.SPLITK_CASES if N % 4 == 0]
    assert all(any(l[i] for l in loops) for i in range(3))
    assert any(G.pad32(K) // G.BK % G.plan(M, N, K).kt_per_split for M, N, K in G.SPLITK_CASES)


def test_tile_table_covers_every_value_with_every_bn():
    by_bn = {}
    for M, N, K, pack, _ in G.TILE_CASES:
        by_bn.setdefault(G.plan(M, N, K).bn, []).append((M, K, pack))
    assert sorted(by_bn) == [32, 64, 128]
    for bn, v in by_bn.items():
        assert {m for m, _, _ in v} == set(G.TILE_MS) and {k for _, k, _ in v} == set(G.TILE_KS), bn
        assert {p for _, _, p in v} == {'kn', 'nk'}, bn
    assert {N for _, N, _, _, _ in G.TILE_CASES} == set(G.TILE_NS)
