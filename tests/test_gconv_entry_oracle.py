"""The oracle of the fp32 gather-convolution entry points (tests/gconv_entry_oracle.py) checked against itself on the host:
the bounds admit an honest fp32 implementation at every shape and precision the GPU test runs
(tests/test_gpu_gconv_entry.py) and reject each planted error on every shape it applies to, the restatements equal the
reference operators (oracle/modules.graph_conv on a real tree, torch's conv3d and its autograd on a 4^3 grid), and the
path predictor names the path of hand-listed calls."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gconv_entry_oracle as O
import gemm_oracle as GM
import graph_oracle as GR

WORST = {}
_REF = {}
WS = GM.WS_DEFAULT


def _ref(shape, **kw):
    key = (shape[0], str(sorted(kw.items())))
    if key not in _REF:
        c = O.case(shape, **kw)
        _REF[key] = (c, O.reference(c))
    return _REF[key]


def _plans(c, stats=False, chunk=None):
    """the launches of a case: its own path with the default workspace, or 128-row col chunks"""
    if chunk:
        return O.launch_plan(False, c.n, c.cout, c.Kp, O.ws_for_chunk(c.Kp, chunk), stats)
    return O.launch_plan(O.fast_path(c.cin, c.cin), c.n, c.cout, c.Kp, WS, stats)


def _worst(key, w):
    WORST[key] = max(WORST.get(key, 0.0), w)


@pytest.mark.parametrize('prec', O.PRECISIONS)
@pytest.mark.parametrize('shape', O.ALL_FWD, ids=lambda s: s[0])
def test_forward_emulation_within_the_bound(shape, prec):
    with torch.no_grad():
        c, r = _ref(shape)
        for plans in (_plans(c), _plans(c, stats=True), _plans(c, chunk=128)):
            w = O.assert_close(O.emulate(c, prec, plans), r['ref'], r['S'], O.bound(prec, r, plans), '%s %d' % (shape[0], prec))
            _worst(('fwd', prec), w)


@pytest.mark.parametrize('mut', O.MUTATIONS)
def test_forward_planted_error_exceeds_the_bound(mut):
    """on at least one element of EVERY shape and precision the error applies to"""
    seen = 0
    with torch.no_grad():
        for shape in O.ALL_FWD:
            c, r = _ref(shape)
            if not O.applies(mut, c):
                continue
            for prec in O.PRECISIONS:
                plans = _plans(c, stats=True)
                seen += 1
                with pytest.raises(AssertionError, match='worst'):
                    O.assert_close(O.emulate(c, prec, plans, mut=mut), r['ref'], r['S'], O.bound(prec, r, plans),
                                   '%s %s %d' % (mut, shape[0], prec))
    assert seen >= 9, (mut, seen)


@pytest.mark.parametrize('prec', O.PRECISIONS)
def test_backward_emulation_and_the_unweighted_gather(prec):
    with torch.no_grad():
        for shape in O.BWD_SHAPES:
            c = O.bwd_case(shape)
            r = O.reference_bwd(c)
            plans = O.launch_plan(O.fast_path(c.cout, c.cout), c.n, c.cin, c.Kp, WS, False)
            b = O.bound(prec, r, plans)
            _worst(('bwd', prec), O.assert_close(O.emulate_bwd(c, prec, plans), r['ref'], r['S'], b, shape[0]))
            # weighted and multi-row segments coincide
            Ls = np.diff(c.rev_ptr)
            if c.n > 1:
                assert any(Ls[s] > 1 and (c.w[c.rev_ptr[s]:c.rev_ptr[s + 1]] != 1).any() for s in range(len(Ls)))
            with pytest.raises(AssertionError, match='worst'):
                O.assert_close(O.emulate_bwd(c, prec, plans, 'unweighted'), r['ref'], r['S'], b, shape[0])


@pytest.mark.parametrize('prec', O.PRECISIONS)
def test_grid_emulation_and_the_padded_tap(prec):
    with torch.no_grad():
        for mode, d, B in O.GRID_TABLES:
            for cin, cout in O.GRID_WIDTHS:
                c = O.grid_case(mode, d, B, cin, cout)
                r = O.reference_grid(c)
                plans = O.launch_plan(O.fast_path(cin, cin), c.n_out, cout, c.Kp, WS, False)
                b = O.bound(prec, r, plans)
                what = 'grid %d %d %d %d' % (mode, d, B, cin)
                _worst(('grid', prec), O.assert_close(O.emulate_grid(c, prec, plans), r['ref'], r['S'], b, what))
                if bool((c.tab == c.n_in).any()):
                    with pytest.raises(AssertionError, match='worst'):
                        O.assert_close(O.emulate_grid(c, prec, plans, mut='pad_row0'), r['ref'], r['S'], b, what)
                rb = O.reference_grid_bwd(c)
                plans = O.launch_plan(O.fast_path(cout, cout), c.n_in, cin, c.KpT, WS, False)
                _worst(('grid_bwd', prec), O.assert_close(O.emulate_grid_bwd(c, prec, plans), rb['ref'], rb['S'],
                                                          O.bound(prec, rb, plans), what + ' bwd'))


def test_gather_mean_bound():
    seg_ptr, col = GR.hand_csr(5, 40, sizes=O.GATHER_MEAN_SIZES)
    x = GM.operand((40, 8), 6)
    ref, b = O.gather_mean(x, seg_ptr, col)
    got = O._serial_mean(x, seg_ptr, col)
    assert bool(((got.double() - ref).abs() <= b).all())
    L = np.diff(seg_ptr)
    assert bool((b[torch.from_numpy(L <= 1)] == 0).all())                 # a copy / a zero row: exact
    bad = O._serial_mean(x, seg_ptr, col, count_plus=1.0)
    assert not bool(((bad.double() - ref).abs() <= b).all())


def test_stats_bound_admits_fp32_and_rejects_a_skipped_row():
    with torch.no_grad():
        c, r = _ref(O.STATS_SHAPE_V4, cuts=O.STATS_CUTS)
        assert c.B == 5 and int((c.bid == 2).sum()) == 0
        y = O.emulate(c, 1, _plans(c, stats=True))
        s, _ = O.stats_sums(y, c.bid, c.B)
        for route in O.STATS_DEPTH:
            bS, bQ = O.stats_bound(y, c.bid, c.B, route)
            got = O.emulate_stats(y, c.bid, c.B, route)
            assert bool(((got[:, :, 0] - s[:, :, 0]).abs() <= bS).all()) and bool(((got[:, :, 1] - s[:, :, 1]).abs() <= bQ).all())
            bad = O.emulate_stats(y, c.bid, c.B, route, 'skip_after_boundary')
            for b in (1, 3, 4):                                            # every element that starts after a boundary
                assert not bool(((bad[b, :, 0] - s[b, :, 0]).abs() <= bS[b]).all())
                assert not bool(((bad[b, :, 1] - s[b, :, 1]).abs() <= bQ[b]).all())


def test_restatement_equals_the_reference_graph_conv():
    """oracle/modules.graph_conv on a real dual-octree graph (float64), node types included"""
    from oracle import modules as OM
    _, o_doc = GR.tree('full_face')
    d = 3
    g = o_doc.graph[d]
    seg_ptr, col = GR.csr_of_oracle(o_doc, d)
    n = int(g['node_type'].shape[0])
    nt = int(g['node_type'].max()) + 1
    assert nt > 1 and (np.diff(seg_ptr) > 1).any()
    c = O.make_case(n, 5, nt, 6, 3, csr=(seg_ptr, col), node_type=g['node_type'].numpy().astype(np.uint8))
    r = O.reference(c, emb=False, res=False)
    want = OM.graph_conv(c.x.double(), o_doc, d, c.W.double(), c.bias.double(), n_node_type=nt)
    assert float((r['ref'] - want).abs().max()) <= 1e-6 * float(r['S'].max())       # tf is rounded to fp32
    c0 = O.make_case(n, 5, 0, 6, 3, csr=(seg_ptr, col))
    want0 = OM.graph_conv(c0.x.double(), o_doc, d, c0.W.double(), None, n_node_type=0)
    assert float((O.reference(c0, False, False, False)['ref'] - want0).abs().max()) <= 1e-12 * float(r['S'].max())
    # backward: autograd of the same operator, through the reverse CSR of graph_oracle.reverse
    dy = GM.operand((n, 6), 9).double()
    with torch.enable_grad():                        # (other test modules switch autograd off process-wide)
        xg = c0.x.double().requires_grad_(True)
        (OM.graph_conv(xg, o_doc, d, c0.W.double(), None, n_node_type=0) * dy).sum().backward()
    rev_ptr, rev_row, rev_w = GR.reverse(seg_ptr, col, n)
    val, _ = O.seg_means(dy, rev_ptr, rev_row, rev_w)
    WT = c0.W.double().view(7, 5, 6).permute(0, 2, 1).reshape(42, 5)
    assert float((val.view(n, 42) @ WT - xg.grad).abs().max()) <= 1e-6 * float(xg.grad.abs().max())   # rev_w is fp32


def test_restatement_equals_conv3d_and_its_autograd():
    """mode 0 at depth 2, one batch element: a 4^3 grid in Morton order against torch's conv3d"""
    from gridtab_oracle import _morton
    c = O.make_grid_case(0, 2, 1, 3, 5, 1)
    mo = torch.tensor(_morton(2)).reshape(-1)                               # x-major lattice index -> row
    with torch.enable_grad():
        xl = c.x.double()[mo].view(4, 4, 4, 3).permute(3, 0, 1, 2)[None].requires_grad_(True)
        y = F.conv3d(xl, c.weight.double(), c.bias.double(), padding=1)
    want = y[0].detach().permute(1, 2, 3, 0).reshape(64, 5)
    r = O.reference_grid(c, emb=False, res=False)
    assert float((r['ref'][mo] - want).abs().max()) <= 1e-12 * float(r['S'].max())
    dyl = torch.zeros(64, 5, dtype=torch.float64)
    dyl[:] = c.dy.double()[mo]
    with torch.enable_grad():
        (y * dyl.view(4, 4, 4, 5).permute(3, 0, 1, 2)[None]).sum().backward()
    rb = O.reference_grid_bwd(c)
    assert float((rb['ref'][mo] - xl.grad[0].permute(1, 2, 3, 0).reshape(64, 3)).abs().max()) <= 1e-12 * float(rb['S'].max())


def test_path_predictor_and_chunks():
    assert O.fast_path(64, 64) and O.fast_path(32, 96)
    assert not O.fast_path(24, 24) and not O.fast_path(3, 4) and not O.fast_path(64, 66) and not O.fast_path(64, 64, x_off=4)
    assert not O.fast_path(64, 64, ext=False) and not O.fast_path(64, 64, aux=False) and not O.fast_path(64, 64, aux_off=4)
    assert O.col_chunk(512, 588 * 512)[0] == 128 and O.col_chunk(512, 588 * 512 - 2048)[0] == 0       # ofx.h: 588 * Kp
    ws = O.ws_for_chunk(512, 128)
    assert [p[:2] for p in O.launch_plan(False, 300, 36, 512, ws, True)] == [(0, 128), (128, 128), (256, 44)]
    assert all(p[2].nsplit == 1 for p in O.launch_plan(False, 300, 36, 512, ws, True))
    assert O.launch_plan(True, 300, 36, 512, WS, False)[0][2].nsplit > 1
    assert O.launch_plan(True, 300, 36, 512, WS, True)[0][2].nsplit == 1
    assert O.stats_route(True, 300, 36, 512, WS, True) == 'partials'
    assert O.stats_route(True, 300, 36, 512, 5 * 36 * 8 - 16, True) == 'atomic_float4'
    assert O.stats_route(True, 300, 36, 512, 5 * 36 * 8, True) == 'partials'
    assert O.stats_route(True, 300, 3, 512, WS, False) == 'atomic' and O.stats_route(False, 300, 36, 512, ws, True) == 'partials'
    assert O.stats_route(True, 300, 36, 512, 0, True) == 'atomic_float4'
    assert (O.nt_pad(0), O.nt_pad(1), O.nt_pad(4), O.nt_pad(5)) == (0, 0, 32, 64)
    assert O.packed_k(3, 5) == 96 and O.packed_k(64, 4) == 480 and O.packed_k(3, 0, 27) == 96
    # the label cuts of the statistics cases: inside the first wave tile, inside the second chunk, on a chunk boundary
    cuts = O.STATS_CUTS
    assert 0 < cuts[1] < 64 and 128 < cuts[2] < 256 and 256 in cuts and cuts[2] == cuts[3]


def test_zz_worst_ratio_of_the_emulation():
    print('worst ratio to the bound, host emulation:', {k: round(v, 4) for k, v in sorted(WORST.items(), key=str)})
    assert all(v <= 1.0 for v in WORST.values())


# ------------------------------------------------------------------------------------------------ narrow convolutions
def test_narrow_in_emulation_mutations_and_the_byte_counter():
    with torch.no_grad():
        for i, (cin, nt) in enumerate(O.NARROW_IN_WIDTHS):
            c = O.make_narrow_in(65, cin, nt, 64 if i % 2 else 128, 20 + i)
            r = O.reference_narrow_in(c)
            for tab in (False, True):
                b = O.bound_narrow_in(r, O.narrow_inst(cin, nt, tab)[0])
                _worst(('narrow_in', tab), O.assert_close(O.emulate_narrow_in(c, tab), r['ref'], r['S'], b, str((cin, nt, tab))))
                for mut in ('drop_dir', 'wrong_count', 'bias_twice'):
                    with pytest.raises(AssertionError, match='worst'):
                        O.assert_close(O.emulate_narrow_in(c, tab, mut=mut), r['ref'], r['S'], b, mut)
        assert {O.narrow_inst(ci, nt, False) for ci, nt in O.NARROW_IN_WIDTHS} == {(k, ci) for k in (64, 96) for ci in (4, 8)}
        assert {O.narrow_inst(ci, nt, True) for ci, nt in O.NARROW_IN_WIDTHS} == {(k, ci) for k in (64, 72, 96) for ci in (4, 8)}
        assert all(7 * (ci + nt) > 96 for ci, nt in O.NARROW_IN_REFUSED)
        # the header's limit of _tab: 255 rows of one type in a segment are exact, 256 read back as 0 of it and 1 of the next
        for size, ok in ((255, True), (256, False)):
            c = O.make_narrow_in(300, 3, 5, 64, 7, sizes=(0, 1, 2, 8, size, 3), one_type=size)
            r = O.reference_narrow_in(c)
            b = O.bound_narrow_in(r, 64)
            O.assert_close(O.emulate_narrow_in(c, False), r['ref'], r['S'], b, 'narrow_in %d' % size)
            if ok:
                O.assert_close(O.emulate_narrow_in(c, True), r['ref'], r['S'], b, 'tab 255')
            else:
                with pytest.raises(AssertionError, match='worst'):
                    O.assert_close(O.emulate_narrow_in(c, True), r['ref'], r['S'], b, 'tab 256')
        assert O._byte_counts(np.array([[256, 0, 0, 0, 0, 0, 0, 0]])).tolist() == [[0, 1, 0, 0, 0, 0, 0, 0]]
        assert O._byte_counts(np.array([[255, 3, 0, 0, 0, 0, 0, 7]])).tolist() == [[255, 3, 0, 0, 0, 0, 0, 7]]


def test_narrow_in_equals_the_forward_restatement_and_stats_depth():
    """the raw-weight restatement is the packed one (nt > 1), and the narrow statistics depth admits fp32"""
    with torch.no_grad():
        c = O.make_narrow_in(65, 3, 5, 64, 3)
        f = O.make_case(65, 3, 5, 64, 3, csr=(c.seg_ptr, c.col), node_type=c.node_type)
        f.x, f.W, f.bias = c.x, c.W, c.bias
        f.Wk = O.kernel_order(c.W, 3, 5)
        r, rf = O.reference_narrow_in(c), O.reference(f, True, False, False)
        assert float((r['ref'] - rf['ref']).abs().max()) <= 1e-6 * float(r['S'].max())            # f.tf is rounded to fp32
        y = O.emulate_narrow_in(c)
        s, _ = O.stats_sums(y, c.bid, c.B)
        bS, bQ = O.stats_bound(y, c.bid, c.B, 'narrow')
        got = O.emulate_stats(y, c.bid, c.B, 'atomic')                      # 32-row serial runs: deeper than the kernel's 18
        bS32, bQ32 = O.stats_bound(y, c.bid, c.B, 'atomic')
        assert bool(((got[:, :, 0] - s[:, :, 0]).abs() <= bS32).all()) and bool((bS < bS32).all() and (bQ <= bQ32).all())
        got = O.emulate_stats(y, c.bid, c.B, 'partials')
        assert bool(((got[:, :, 0] - s[:, :, 0]).abs() <= bS).all()) and bool(((got[:, :, 1] - s[:, :, 1]).abs() <= bQ).all())
        bad = O.emulate_stats(y, c.bid, c.B, 'partials', 'skip_after_boundary')
        assert not bool(((bad[1, :, 0] - s[1, :, 0]).abs() <= bS[1]).all())


def test_narrow_out_pack_type_term_and_aggregate():
    with torch.no_grad():
        seg_ptr, col = GR.hand_csr(3, 100, sizes=(0, 1, 2, 256, 1000, 3))
        for cout in range(1, 9):
            C, nt = 16, 5
            W = GM.weight(7 * (C + nt), cout, 40 + cout)
            for pw in (7 * cout, 32, 64):
                if pw < 7 * cout:
                    continue
                Wd = O.pack_reference(W, C, nt, cout, pw)
                assert float(Wd[3, 2 * cout + cout - 1]) == float(W[2 * (C + nt) + 3, cout - 1])
                assert bool((Wd[:, 7 * cout:] == 0).all())
            ty = np.arange(100).astype(np.uint8) % nt
            tf = torch.from_numpy(GR.type_frac(seg_ptr, col, ty, nt)[0]).reshape(100, 7 * nt).float()
            bias = GM.operand((cout,), 50 + cout)
            ref, b = O.type_term(tf, nt, W, C, cout, bias)
            tt = O.emulate_type_term(tf, nt, W, C, cout, bias)
            assert bool(((tt.double() - ref).abs() <= b).all())
            assert not bool(((tt.double() + bias.double() - ref).abs() <= b).all())                 # the bias added twice
            ref0, b0 = O.type_term(tf, 0, W[:7 * C], C, cout, None)
            assert float(ref0.abs().max()) == 0.0 and float(b0.abs().max()) == 0.0
            P = GM.operand((100, 64), 60 + cout)
            ref, b, S = O.reference_narrow_out(P, cout, seg_ptr, col, tt)
            got = O.emulate_narrow_out(P, cout, seg_ptr, col, tt)
            _worst(('narrow_out', cout), O.assert_close(got, ref, S, b, 'narrow_out %d' % cout))
            with pytest.raises(AssertionError, match='worst'):
                O.assert_close(O.emulate_narrow_out(P, cout, seg_ptr, col, tt, 'swap_dirs'), ref, S, b, 'swap')
