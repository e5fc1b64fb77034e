"""The oracle of the planes GraphConv entry points (tests/gconv_planes_oracle.py) checked against itself on the host: the
bounds admit an honest fp32 implementation at every shape and mode the GPU test runs (tests/test_gpu_gconv_planes_entry.py)
and reject each planted error on at least one element of every shape it applies to -- the condition that makes the GPU
test meaningful --, the pack reference round-trips, and the reference equals a plain dense restatement."""
import pytest
import torch

import gconv_planes_oracle as O
import gn_oracle as GN

torch.set_grad_enabled(False)
WORST = {}
_REF = {}


def _ref(shape, mode):
    key = (shape[0], mode)
    if key not in _REF:
        c = O.case(shape, mode)
        _REF[key] = (c, O.reference(c))
    return _REF[key]


def _bound(c, r, pieces):
    return O.bound(c.mode, r, c.nkt * O.chunk(c.mode), pieces, c.multi_mask)


@pytest.mark.parametrize('mode', O.MODES)
@pytest.mark.parametrize('shape', O.ALL_SHAPES, ids=lambda s: s[0])
def test_emulation_within_the_bound(shape, mode):
    c, r = _ref(shape, mode)
    for pieces in (1, 3):
        w = O.assert_close(O.emulate(c, pieces), r['ref'], r['S'], _bound(c, r, pieces), '%s mode %d' % (shape[0], mode))
        WORST[mode] = max(WORST.get(mode, 0.0), w)


def test_emulation_within_the_bound_with_labels_planted():
    for mode in O.MODES:
        c = O.case(O.LABEL_SHAPE, mode, cuts=O.LABEL_CUTS)
        r = O.reference(c)
        assert c.B == 6
        O.assert_close(O.emulate(c), r['ref'], r['S'], _bound(c, r, 1), 'labels mode %d' % mode)


@pytest.mark.parametrize('mut', O.MUTATIONS)
def test_planted_error_exceeds_the_bound(mut):
    """on at least one element of EVERY shape and mode the error applies to"""
    seen = 0
    for shape in O.ALL_SHAPES:
        for mode in O.MODES:
            c, r = _ref(shape, mode)
            if not O.applies(mut, c):
                continue
            seen += 1
            with pytest.raises(AssertionError, match='worst'):
                O.assert_close(O.emulate(c, 1, mut), r['ref'], r['S'], _bound(c, r, 1), '%s %s mode %d' % (mut, shape[0], mode))
    assert seen >= 6, (mut, seen)


def test_lo_half_errors_show_at_the_probe():
    """the dropped cross terms are rejected at the planted element, not by accident elsewhere"""
    for mode in (3, 2):
        c, r = _ref(O.LADDER_SHAPE, mode)
        for mut in ('drop_alo_whi', 'drop_ahi_wlo', 'lo_hi'):
            with pytest.raises(AssertionError, match=r'\(m, n\) = \(%d, %d\)' % c.probe):
                O.assert_close(O.emulate(c, 1, mut), r['ref'], r['S'], _bound(c, r, 1))


def test_aux_mask_matters():
    """without the aux term of its slots the bound must be smaller exactly there"""
    c, r = _ref(O.AUX_SHAPES[0], 2)
    full = _bound(c, r, 1)
    none = O.bound(c.mode, r, c.nkt * O.chunk(c.mode), 1, torch.zeros_like(c.multi_mask))
    has = c.multi_mask.any(1)
    assert bool(has.any()) and bool((~has).any())
    assert torch.equal(full[~has], none[~has]) and bool((full[has] > none[has]).all())
    c0, r0 = _ref(O.AUX_SHAPES[1], 2)
    assert len(c0.multi) == 0 and not bool(c0.multi_mask.any())


@pytest.mark.parametrize('mode', O.MODES)
def test_aux_rows(mode):
    """the bytes of the float64 mean decode to within aux_err of it; row 0 is zero bytes; segments of 2, 8 and 9"""
    c = O.case(O.AUX_SHAPES[0], mode)
    mean, raw = O.aux(c)
    L = sorted({int(c.seg_ptr[s + 1] - c.seg_ptr[s]) for s in c.multi.tolist()})
    assert L == [2, 8, 9]
    assert int(raw[0].sum()) == 0 and float(mean[0].abs().max()) == 0.0
    assert bool(((GN.decode(raw, c.cin, mode) - mean).abs() <= O.aux_err(c))[1:].all())
    serial = GN.aux_rows(c.xd, torch.from_numpy(c.seg_ptr), torch.from_numpy(c.col), c.multi)      # another summation order
    assert bool(((mean - serial).abs() <= 2.0 ** -48 * c.xd.abs().max()).all())


@pytest.mark.parametrize('mode', O.MODES)
@pytest.mark.parametrize('nt', O.PACK_NTS)
def test_pack_reference_round_trip(nt, mode):
    """decode(pack_reference) is W s in kernel order to within the format's split error; trailer [1 / s, s]; sizes"""
    cin, cout = 64, 9
    K = 7 * (cin + O.ntc(nt))
    W = torch.randn(K, cout, generator=torch.Generator().manual_seed(nt + 10 * mode)) * 3.0
    W[5, 2] = O.PROBE_W
    raw = O.pack_reference(W, cin, nt, cout, mode)
    assert raw.numel() == O.packed_bytes(cin, nt, cout, mode)
    ch = O.chunk(mode)
    assert O.ktiles(cin, nt, mode) == 7 * cin // ch + (7 * O.ntc(nt) + ch - 1) // ch
    s = O.pack_scale(W, mode)
    assert (s == 1.0) == (mode == 2)
    tr = raw[-O.LINE:].view(torch.float32)
    assert float(tr[0]) == 1.0 / s and float(tr[1]) == s
    want = O.kernel_order(W, cin, nt, mode).double() * s
    got = O.pack_decode(raw, cin, nt, cout, mode)
    assert bool(((got - want).abs() <= O.split_err(mode, want.abs())).all())
    assert float(got[7 * cin + 7 * O.ntc(nt):].abs().max() if got.shape[0] > 7 * cin + 7 * O.ntc(nt) else 0.0) == 0.0
    # k order: feature (dir, c) at dir * cin + c, type (dir, t) at 7 cin + dir * ntc + t
    t = O.ntc(nt)
    assert abs(float(got[0 * cin + 5, 2]) - O.PROBE_W * s) <= float(O.split_err(mode, torch.tensor(O.PROBE_W * s)))
    if t:
        d, ty = 3, t - 1
        assert abs(float(got[7 * cin + d * t + ty, 4]) - float(W[d * (cin + t) + cin + ty, 4]) * s) <= \
            float(O.split_err(mode, W[d * (cin + t) + cin + ty, 4].abs().double() * s))
    if O.pairs(mode):                                                  # [hi | lo], not [lo | hi]
        hi = GN.decode_hi(raw[:O.LINE * cout].view(cout, O.LINE), ch, mode)
        rnd = {3: 2.0 ** -11, 2: 2.0 ** -8}[mode]
        assert bool(((hi - want[:ch].t()).abs() <= rnd * want[:ch].t().abs() + 2.0 ** -24).all())


def test_reference_equals_dense_restatement():
    """col_data built slot by slot with python loops, then @ W"""
    for mode in O.MODES:
        c = O.make_case(37, 64, 3, 5, mode, 11, sizes=(0, 1, 2, 3, 2, 1))
        r = O.reference(c)
        cd = torch.zeros(c.n, c.K, dtype=torch.float64)
        w = c.cin + c.ntc
        for m in range(c.n):
            for d in range(7):
                s = m * 7 + d
                a, e = int(c.seg_ptr[s]), int(c.seg_ptr[s + 1])
                if e > a:
                    cd[m, d * w:d * w + c.cin] = c.xd[c.col[a:e]].sum(0) / (e - a)
                cd[m, d * w + c.cin:(d + 1) * w] = c.tfd[m, d * c.ntc:(d + 1) * c.ntc]
        want = cd @ c.W.double() + c.bias.double() + c.emb.double()[c.bid.long()] + c.res.double()
        assert float((r['ref'] - want).abs().max()) <= 1e-12 * float(r['S'].max())
        assert float((O.col_data(c) - cd).abs().max()) <= 1e-14 * float(cd.abs().max())


def test_stats_bound_admits_fp32_and_rejects_a_dropped_row():
    c, r = _ref(O.LABEL_SHAPE, 3)
    y = O.emulate(c)
    s, _ = O.stats_sums(y, c.bid, c.B)
    for path, run in (('float4', 8), ('scalar', 32)):
        bS, bQ = O.stats_bound(y, c.bid, c.B, path)
        got = torch.zeros_like(s)
        for b in range(c.B):                                   # fp32 runs of `run` rows, added in fp64
            rows = y[c.bid == b]
            for i in range(0, rows.shape[0], run):
                accs, accq = torch.zeros(c.cout), torch.zeros(c.cout)
                for v in rows[i:i + run]:
                    accs, accq = accs + v, accq + v * v
                got[b, :, 0] += accs.double()
                got[b, :, 1] += accq.double()
        assert bool(((got[:, :, 0] - s[:, :, 0]).abs() <= bS).all()) and bool(((got[:, :, 1] - s[:, :, 1]).abs() <= bQ).all())
        drop = s.clone()
        drop[0, :, 0] -= y[0].double()
        drop[0, :, 1] -= y[0].double() ** 2
        assert not bool(((drop[:, :, 0] - s[:, :, 0]).abs() <= bS).all())
        assert not bool(((drop[:, :, 1] - s[:, :, 1]).abs() <= bQ).all())


def test_shape_tables():
    """what the GPU test relies on: partial last tiles and waves, both NI, the type rows crossing a k tile, plan_pieces"""
    for shape in O.ALL_SHAPES:
        n = shape[1]
        assert n % 64 and n % 128 and n % 256 and n > 256
    assert {O.ni_of(s[4]) for s in O.SCALAR_WIDTHS} == {1, 2} and all(s[4] % 4 for s in O.SCALAR_WIDTHS[:1])
    assert not O.is_vec4(3, 3) and not O.is_vec4(70, 70) and O.is_vec4(128, 128, ldr=128, lde=128)
    assert not O.is_vec4(128, 129, ldr=128, lde=128) and not O.is_vec4(128, 128, out_off=4, ldr=128, lde=128)
    assert not O.is_vec4(128, 128, ldr=129, lde=128) and not O.is_vec4(128, 128, ldr=128, lde=129)
    assert not O.is_vec4(128, 128, ldr=128, lde=128, res_off=4) and not O.is_vec4(128, 128, ldr=128, lde=128, bias_off=4)
    assert O.type_tiles(9, 3) == 2 and O.type_tiles(9, 1) == 1 and O.type_tiles(10, 1) == 2 and O.type_tiles(5, 2) == 2
    assert O.type_tiles(1, 3) == 0 and O.type_tiles(4, 3) == 1
    # 8 blocks, q = 10 units, boundaries 0 10 ... 80 over tiles of 16 k-steps: tile 0 cut once, tile 1 (16..32) twice
    plan = [8, 10, 0, 80, 0] + [10 * b for b in range(9)]
    assert O.plan_pieces(plan, 16) == (3, True) and O.plan_pieces([2, 16, 0, 32, 0, 0, 16, 32], 16) == (1, False)


def test_zz_worst_ratio_of_the_emulation():
    print('worst ratio to the bound, host emulation:', {O.MODE_NAME[k]: round(v, 4) for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())
