"""tests/gn_oracle.py against itself, on the host: every bound the GPU tests of the GroupNorm forward entry points use
(tests/test_gpu_gn_entry.py) must ACCEPT an honest float32 evaluation of the same case and must REJECT the errors a
subtly wrong kernel makes -- a row counted into the neighbouring batch element, a row dropped, one group's statistics
used for all four channels of a float4, count_eps left out, hi / lo halves swapped, a chunk's line taken from the next
chunk, an aux row divided by 4 instead of its segment length.  The cases, inputs and constants are the GPU file's."""
import pytest
import torch
import torch.nn.functional as F

import gn_oracle as O

torch.set_grad_enabled(False)

G_ACTS = (None, 'silu', 'gelu')


# ------------------------------------------------------------------------------------------------ statistics
def _stats_ok(got, s, mag, run, what):
    cS, cQ = O.sums_c(run)
    return max(O.assert_close(got[:, :, 0], s[:, :, 0], mag[:, :, 0], cS, what + ' sum'),
               O.assert_close(got[:, :, 1], s[:, :, 1], mag[:, :, 1], cQ, what + ' sum of squares'))


@pytest.mark.parametrize('C', O.STATS_C)
def test_float32_sums_pass(C):
    for i, sizes in enumerate(O.STATS_LAYOUTS):
        x, bid = O.make_x(sizes, C, C // 4, 1000 * C + i)
        s, mag = O.sums(x, bid, len(sizes))
        run = O.stats_run(C)
        _stats_ok(O.sums(x, bid, len(sizes), torch.float32, run)[0], s, mag, run, 'C %d %r' % (C, sizes))
        for b, nb in enumerate(sizes):                             # an empty element is exactly zero
            assert nb > 0 or not bool(s[b].any())


@pytest.mark.parametrize('C,n,rpb', O.STATS_BIG)
def test_float32_sums_of_the_large_blocks_pass(C, n, rpb):
    x, bid = O.make_x((n,), C, C // 4, C + n)
    s, mag = O.sums(x, bid, 1)
    run = O.stats_run(C, rpb)
    assert run == {256: 32, 1024: 192}[C]
    used = _stats_ok(O.sums(x, bid, 1, torch.float32, run)[0], s, mag, run, 'C %d n %d' % (C, n))
    print('C %d n %d run %d: float32 uses %.3f of the bound' % (C, n, run, used))


@pytest.mark.parametrize('plant', ['neighbour_element', 'dropped_row'])
@pytest.mark.parametrize('C,sizes', [(4, (1, 0, 62)), (96, (101, 57, 99)), (1024, (9, 9, 9, 9, 9, 9, 10)), (256, (4097,))])
def test_planted_statistics_errors_fail(C, sizes, plant):
    x, bid = O.make_x(sizes, C, C // 4, 5 * C)
    B = len(sizes) + 1                                             # (a spare element for the single-element case)
    s, mag = O.sums(x, bid, B)
    run = O.stats_run(C, 128 if len(sizes) == 1 else 64)
    _stats_ok(O.sums(x, bid, B, torch.float32, run)[0], s, mag, run, 'honest')
    if plant == 'neighbour_element':
        bad = bid.clone()
        r = int((bid == bid[-1]).nonzero()[0])                     # first row of the last element ...
        bad[r] = bid[-1] - 1 if len(sizes) > 1 else 1              # ... counted into the one before it
        got = O.sums(x, bad, B, torch.float32, run)[0]
    else:
        keep = torch.ones(len(bid), dtype=torch.bool)
        keep[len(bid) // 2] = False
        got = O.sums(x[keep], bid[keep], B, torch.float32, run)[0]
    with pytest.raises(AssertionError):
        _stats_ok(got, s, mag, run, plant)


# ------------------------------------------------------------------------------------------------ finalize
FIN_CASES = [(C, C // cpg, ce) for C, cpgs in ((12, (1, 2, 3, 4, 6)), (96, (1, 2, 3, 4, 6, 32))) for cpg in cpgs
             for ce in (O.EPS, 0.0)]


@pytest.mark.parametrize('C,groups,count_eps', FIN_CASES)
def test_float32_finalize_passes_and_a_missing_count_eps_fails(C, groups, count_eps):
    sizes = (5, 0, 40) if count_eps else (5, 3, 40)
    x, bid = O.make_x(sizes, C, groups, C + groups)
    s, _ = O.sums(x, bid, 3)
    cnt = O.counts(sizes)
    m, r = O.finalize(s[:, :, 0], s[:, :, 1], cnt, C, groups, O.EPS, count_eps)
    m32, r32 = O.finalize(s[:, :, 0], s[:, :, 1], cnt, C, groups, O.EPS, count_eps, torch.float32)
    cm, cr = O.finalize_c(s[:, :, 0], s[:, :, 1], cnt, C, groups, O.EPS, count_eps)
    assert float(cm.max()) < 1.1 and float(cr.max()) < 1.1         # the fp32 roundings of the two results, nothing else
    O.assert_close(m32, m, m.abs(), cm, 'mean')
    O.assert_close(r32, r, r, cr, 'rstd')
    cpg = C // groups
    assert abs(float(r[0, 0]) * O.f32(O.EPS) ** 0.5 - 1) < 1e-6    # the constant group: rstd = 1 / sqrt(eps)
    if count_eps:
        assert float(m[1].abs().max()) == 0.0 and abs(float(r[1, 0]) * O.f32(O.EPS) ** 0.5 - 1) < 1e-12     # count 0
        other = O.finalize(s[:, :, 0], s[:, :, 1], cnt, C, groups, O.EPS, 0.0, torch.float32)
        with pytest.raises(AssertionError):                        # 1e-5 / (5 cpg) of the mean: 2^-24 * 10 and more
            O.assert_close(other[0][0], m[0], m[0].abs(), cm[0], 'count_eps left out of inv')
    # against torch.nn.functional.group_norm's statistics where the two definitions coincide
    if not count_eps:
        xb = x[bid == 2].double().t().reshape(1, C, -1)
        mt = xb.reshape(groups, -1).mean(1)
        vt = xb.reshape(groups, -1).var(1, unbiased=False)
        assert torch.allclose(m[2, ::cpg], mt, rtol=1e-6, atol=1e-9)
        assert torch.allclose(r[2, ::cpg], 1 / torch.sqrt(vt + O.f32(O.EPS)), rtol=1e-6)


def test_finalize_window_is_the_slice_with_the_buffers_pitch():
    C, groups, lo, hi = 128, 32, 32, 96
    sizes = (9, 30)
    x, bid = O.make_x(sizes, C, groups, 3)
    s, _ = O.sums(x, bid, 2)
    full = O.finalize(s[:, :, 0], s[:, :, 1], O.counts(sizes), C, groups, O.EPS, O.EPS)
    win = O.finalize(s[:, lo:, 0], s[:, lo:, 1], O.counts(sizes), hi - lo, (hi - lo) // 4, O.EPS, O.EPS)
    assert torch.equal(win[0], full[0][:, lo:hi]) and torch.equal(win[1], full[1][:, lo:hi])


# ------------------------------------------------------------------------------------------------ apply
def _apply_f32(x, bid, sizes, C, groups, w, b, act, count_eps, run=None):
    """the honest float32 chain: (fp32 sums in runs when `run`, else exact ones) -> rounded mean / rstd -> fp32 apply"""
    B = len(sizes)
    s = O.sums(x, bid, B, torch.float32, run)[0] if run else O.sums(x, bid, B)[0]
    m, r = O.finalize(s[:, :, 0], s[:, :, 1], O.counts(sizes), C, groups, O.EPS, count_eps, torch.float32)
    return O.apply(x, bid, m, r, w, b, act, torch.float32)[0]


@pytest.mark.parametrize('C', sorted(O.APPLY_CPG))
def test_float32_apply_passes(C):
    worst = 0.0
    for cpg in O.APPLY_CPG[C]:
        for li, sizes in enumerate(O.APPLY_LAYOUTS):
            for act in G_ACTS:
                x, bid = O.make_x(sizes, C, C // cpg, C + 10 * cpg + li)
                w, b = O.make_affine(C, C)
                ref, S, c, _, _ = O.apply_reference(x, bid, sizes, C, C // cpg, w, b, act, O.EPS)
                got = _apply_f32(x, bid, sizes, C, C // cpg, w, b, act, O.EPS)
                assert got.dtype == torch.float32
                worst = max(worst, O.assert_close(got, ref, S, c, 'C %d cpg %d %r %s' % (C, cpg, sizes, act)))
    print('C %d: float32 uses %.3f of the bound' % (C, worst))


@pytest.mark.parametrize('cpg', [2, 3])
@pytest.mark.parametrize('act', G_ACTS)
def test_one_group_for_all_four_channels_of_a_float4_fails(cpg, act):
    C, sizes = 12, (21, 20, 22)
    x, bid = O.make_x(sizes, C, C // cpg, 40 + cpg)
    w, b = O.make_affine(C, C)
    ref, S, c, (mean, rstd), _ = O.apply_reference(x, bid, sizes, C, C // cpg, w, b, act, O.EPS)
    m, r = mean.clone(), rstd.clone()
    for c0 in range(0, C, 4):                                      # the middle element only: the fallback's rows
        m[1, c0:c0 + 4], r[1, c0:c0 + 4] = mean[1, c0], rstd[1, c0]
    assert not torch.equal(m, mean)
    O.assert_close(O.apply(x, bid, mean.float(), rstd.float(), w, b, act, torch.float32)[0], ref, S, c, 'honest')
    with pytest.raises(AssertionError):
        O.assert_close(O.apply(x, bid, m.float(), r.float(), w, b, act, torch.float32)[0], ref, S, c, 'one group')


# ------------------------------------------------------------------------------------------------ planes
@pytest.mark.parametrize('mode', [1, 2, 3])
def test_decoders_agree_with_torch(mode):
    C = 128
    g = torch.Generator().manual_seed(mode)
    y = torch.cat([torch.randn(40, C, generator=g) * 3, torch.randn(8, C, generator=g) * 1e-4,
                   torch.randn(8, C, generator=g) * 1e-7])          # normal lo words, subnormal lo words, subnormal hi words
    raw = O.encode(y, mode, 640)
    assert raw.shape == (56, 640) and raw.dtype == torch.uint8
    dec = O.decode(raw, C, mode)
    if mode == 1:
        assert torch.equal(dec, y.to(torch.float16).double())
    else:
        dt = torch.float16 if mode == 3 else torch.bfloat16
        hi = y.to(dt)
        assert torch.equal(dec, hi.double() + (y - hi.float()).to(dt).double())
        # the layout, from the bytes: channel 37 of row 2 is halfword 5 of line 1 (hi) and halfword 32 + 5 (lo)
        line = raw[2, 128:256].contiguous().view(torch.int16).view(dt)
        assert float(line[5]) == float(hi[2, 37]) and float(line[37]) == float((y - hi.float()).to(dt)[2, 37])
    # the documented representation error holds for the honest encoding
    O.assert_close(dec, y.double(), y.double().abs(), O.rep_c(mode, y.double().abs()), 'representation')


@pytest.mark.parametrize('mode,C', O.PLANES_CASES)
def test_float32_planes_pass_and_planted_layout_errors_fail(mode, C):
    groups = C // 4
    w, b = O.make_affine(C, C)
    for li, sizes in reversed(list(enumerate(O.PLANES_LAYOUTS))):
        act = ('silu', 'gelu')[li]
        x, bid = O.make_x(sizes, C, groups, C + mode + li)
        ref, S, c, _, _ = O.apply_reference(x, bid, sizes, C, groups, w, b, act, O.EPS)
        c = c + O.rep_c(mode, S)
        y = _apply_f32(x, bid, sizes, C, groups, w, b, act, O.EPS)
        raw = O.encode(y, mode)
        O.assert_close(O.decode(raw, C, mode), ref, S, c, 'honest planes %r' % (sizes,))
    if mode == 1:
        return
    lines = raw.view(len(bid), C // 32, 2, 64)
    O.assert_close(O.decode_hi(raw, C, mode), ref, S, c + O.HI_C[mode], 'hi half of the honest planes')
    swapped = lines.flip(2).reshape(len(bid), -1)                   # [lo | hi]: hi + lo is unchanged, the first half is not
    O.assert_close(O.decode(swapped, C, mode), ref, S, c, 'the sum cannot tell')
    with pytest.raises(AssertionError):
        O.assert_close(O.decode_hi(swapped, C, mode), ref, S, c + O.HI_C[mode], 'hi / lo swapped')
    if C >= 64:
        moved = torch.roll(lines, -1, 1).reshape(len(bid), -1)      # every chunk's line taken from the next chunk
        with pytest.raises(AssertionError):
            O.assert_close(O.decode(moved, C, mode), ref, S, c, 'neighbouring chunk')


def test_float32_aux_rows_pass_and_a_fixed_divisor_fails():
    seg_ptr, col, multi, bid, sizes = O.aux_case()
    lens = (seg_ptr[multi.long() + 1] - seg_ptr[multi.long()]).tolist()
    assert sorted(set(lens)) == [2, 4, 5, 9] and len(multi) + 1 > 16
    rows = (multi // 7).long()
    assert set(bid[rows].tolist()) == {0, 1}
    for v, s in enumerate(multi.tolist()):                        # sources in the batch element of the segment's row
        assert bool((bid[col[seg_ptr[s]:seg_ptr[s + 1]].long()] == bid[s // 7]).all())
    C, mode = 64, 3
    x, _ = O.make_x(sizes, C, 16, 130)
    w, b = O.make_affine(C, C)
    ref, S, c, _, _ = O.apply_reference(x, bid, sizes, C, 16, w, b, 'silu', O.EPS)
    aref, aS = O.aux_rows(ref, seg_ptr, col, multi), O.aux_rows(S, seg_ptr, col, multi)
    ac = O.aux_c(c, seg_ptr, col, multi) + O.rep_c(mode, aS)
    y = _apply_f32(x, bid, sizes, C, 16, w, b, 'silu', O.EPS)
    a32 = O.aux_rows(y, seg_ptr, col, multi, torch.float32)
    got = O.decode(O.encode(a32, mode), C, mode)
    assert not bool(got[0].any())
    O.assert_close(got[1:], aref[1:], aS[1:], ac[1:], 'honest aux rows')
    bad = got.clone()
    v = lens.index(5)
    bad[1 + v] = got[1 + v] * 5 / 4
    with pytest.raises(AssertionError):
        O.assert_close(bad[1:], aref[1:], aS[1:], ac[1:], 'divided by 4')


# ------------------------------------------------------------------------------------------------ fused rows
@pytest.mark.parametrize('C,groups', O.FUSED_WIDTHS)
def test_float32_fused_rows_pass(C, groups):
    for rows, B in O.FUSED_CASES:
        sizes = (rows,) * B
        cpg = C // groups
        x, bid = O.make_x(sizes, C, groups, C + rows)
        w, b = O.make_affine(C, C)
        cS, cQ = O.fused_c(rows, cpg)
        for count_eps in (O.EPS, 0.0):
            ref, S, c, _, _ = O.apply_reference(x, bid, sizes, C, groups, w, b, 'silu', count_eps, cS, cQ)
            run = -(-rows * cpg // 256)
            # the per-group kernel's chain: a thread's terms are `run` (row, channel) pairs of ONE group; summing whole
            # channels in runs of ceil(run / cpg) rows and the channels in float64 is no longer a chain
            got = _apply_f32(x, bid, sizes, C, groups, w, b, 'silu', count_eps, -(-run // cpg))
            O.assert_close(got, ref, S, c, 'fused C %d G %d rows %d' % (C, groups, rows))
        # count_eps = 0 is torch.nn.functional.group_norm
        t = F.silu(F.group_norm(x.double().view(B, rows, C).transpose(1, 2), groups, w.double(), b.double(), O.f32(O.EPS)))
        ct = O.apply_reference(x, bid, sizes, C, groups, w, b, 'silu', 0.0, slack=1.0)[2]
        O.assert_close(ref, t.transpose(1, 2).reshape(-1, C), S, ct, 'the oracle at count_eps = 0 against torch')
