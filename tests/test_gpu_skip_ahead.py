"""Skip-ahead: the skip half of a decoder res block's conv1(SiLU(GN(cat[h, skip]))) computed before
h exists -- GroupNorm on a channel window (`ofx_gn_apply_planes_window`, `ofx_gn_apply_planes_oct_window`,
`ofx_gn_finalize_window`), the planes GraphConv over a K window planned for a subset of the compute units
(`ofx_graphconv_fwd_planes_cus`), `GraphResBlockEmbed.prepare_skip` and the hr net's second stream.

Tree: depth 5 over a full depth of 3, three elements, the middle one with ONE refined octant -- it owns eight rows of the
depth-4 and of the depth-5 part, so 64-row blocks (and waves of the convolution's tiles) hold rows of three batch elements.
"""
import functools
import inspect
import re

import pytest
import torch

import common as C
import test_gpu_fullwidth as FW
from test_gpu_fullwidth import dev, errors

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _split():
    split = C.random_split_small(3, 3, 31, p=0.45)
    split[1] = -1.0
    split[1, 1, 1, 2, 3] = 1.0
    return split


@functools.lru_cache(maxsize=1)
def _tree():
    from octfusion_amd.dual_octree import DualOctree
    from octfusion_amd.octree import split2octree_small
    from oracle import dual_octree as OD, sampler as OS
    split = _split()
    doc = DualOctree(split2octree_small(split.to(dev()), 5, 3))
    o_doc = OD.OracleDualOctree(OS.split2octree_small(split, 5, 3))
    o_doc.post_processing_for_docnn()
    for d in (4, 5):
        bid = o_doc.batch_id(d)
        assert max(int(torch.unique(bid[i:i + 64]).numel()) for i in range(0, bid.numel(), 64)) == 3
    return doc, o_doc


def _layer_bound():
    """The fp16x3 bound of the per-layer sweep (tests/test_gpu_fullwidth.py::test_per_layer_sweep), read from its source."""
    m = re.search(r"\(\(([0-9.e-]+) if prec == 'fp16x3' else", inspect.getsource(FW.test_per_layer_sweep))
    assert m, 'the per-layer sweep no longer states its bound this way'
    return float(m.group(1))


def _aux_graph(doc, d, how):
    from octfusion_amd import ops
    seg_ptr, col, _, _ = doc.csr(d)
    _, multi_seg, V = doc.ext(d)
    return ops.AuxGraph(seg_ptr, col, multi_seg, V, doc.oct_plan(d) if how == 'oct' else None,
                        doc.aux_plan(d) if how == 'block' else None)


@pytest.mark.parametrize('Cc,window', [(384, (288, 384)), (256, (128, 256))])
@pytest.mark.parametrize('how,fin', [('oct', 'launch'), ('oct', 'block'), ('block', 'launch')])
def test_gn_window_early_plus_late_is_one_full_call(Cc, window, how, fin):
    """Window [c_lo, C) first -- with the sums of the other channels still garbage -- then [0, c_lo): plane lines and aux
    rows byte for byte those of one full call; octet launch with the finalize launch and with the in-launch finalize,
    block-owned launch (ops.AUX_PLAN = 'block') with the finalize launch."""
    from octfusion_amd import ops
    doc, _ = _tree()
    d, groups = 5, 32
    N, B = doc.csr(d)[2], doc.batch_size
    _, _, V = doc.ext(d)
    sd = C.fill_state_dict([('gnw.weights', (1, Cc)), ('gnw.bias', (1, Cc))])
    w, b = sd['gnw.weights'].to(dev()), sd['gnw.bias'].to(dev())
    bid = doc.batch_id32(d)
    x = ((C.rand_input('gnw_%d' % Cc, N, Cc) * 1.7 + 0.3) + (torch.arange(Cc) % 5) * 2.0).to(dev())
    x = x * (1.0 + 0.5 * bid[:, None].float())
    mode = 3
    saved = (ops.AUX_PLAN, ops.GN_OCT_FINALIZE_MAX_ELEMS, ops.GN_OCT_FINALIZE)
    ops.AUX_PLAN = how
    ops.GN_OCT_FINALIZE = fin == 'block'
    ops.GN_OCT_FINALIZE_MAX_ELEMS = 1 << 40
    try:
        g = _aux_graph(doc, d, how)
        launch, finalize = ops._gn_launch(mode, g, N * Cc, Cc // groups)
        assert launch == how and finalize == (fin == 'launch')
        sums = ops.gn_sums(x, bid, B)
        full = ops.group_norm(x, bid, doc.count(d), B, w, b, groups, 1e-5, 'silu', None, stats=sums, planes=mode, aux_graph=g)
        full_aux = getattr(full, ops.AUX_ATTR)
        c_lo, c_hi = window
        out = torch.full((N, Cc), float('nan'), device=dev())
        aux = torch.full(((V + 2) * Cc * 4,), 0xA5, dtype=torch.uint8, device=dev())
        mean = torch.full((B * Cc,), float('nan'), device=dev()) if finalize else None
        rstd = torch.full((B * Cc,), float('nan'), device=dev()) if finalize else None
        early = sums.clone().view(B, Cc, 2)
        early[:, :c_lo] = float('nan')                       # the h half's sums are not final when the early call runs
        ops.group_norm_window(x, bid, doc.count(d), B, w, b, groups, window, early.view(-1), out, aux, mode, g, 1e-5, 'silu',
                              mean, rstd)
        torch.cuda.synchronize()
        # nothing outside the window was written
        assert bool(torch.isnan(out[:, :c_lo]).all())
        a2 = aux.view(V + 2, Cc * 4)
        assert bool((a2[:V + 1, :c_lo * 4] == 0xA5).all()) and bool((a2[V + 1] == 0xA5).all())
        ops.group_norm_window(x, bid, doc.count(d), B, w, b, groups, (0, c_lo), sums, out, aux, mode, g, 1e-5, 'silu',
                              mean, rstd)
        assert torch.equal(out.view(torch.int32), full.view(torch.int32)), 'plane lines differ'
        assert torch.equal(aux[:(V + 1) * Cc * 4], full_aux[:(V + 1) * Cc * 4]), 'aux rows differ'
    finally:
        ops.AUX_PLAN, ops.GN_OCT_FINALIZE_MAX_ELEMS, ops.GN_OCT_FINALIZE = saved


def test_gn_window_refuses_misaligned_windows():
    from octfusion_amd import _lib, ops
    doc, _ = _tree()
    d, Cc, groups, mode = 5, 384, 32, 3
    N, B = doc.csr(d)[2], doc.batch_size
    _, _, V = doc.ext(d)
    g = _aux_graph(doc, d, 'oct')
    bid = doc.batch_id32(d)
    x = torch.zeros(N, Cc, device=dev())
    w = torch.ones(Cc, device=dev())
    out = torch.empty(N, Cc, device=dev())
    aux = torch.empty((V + 2) * Cc * 4, dtype=torch.uint8, device=dev())
    sums = torch.zeros(B * Cc * 2, dtype=torch.float64, device=dev())
    mean = torch.empty(B * Cc, device=dev())
    # 256: a chunk boundary inside a group (12 channels per group); 300: a group boundary inside a chunk; 384: empty
    for window in ((256, 384), (300, 384), (288, 372), (384, 384), (288, 416), (-96, 96)):
        for how in ('oct', 'block'):
            saved = ops.AUX_PLAN
            ops.AUX_PLAN = how
            try:
                with pytest.raises(_lib.OfxError, match='invalid argument'):
                    ops.group_norm_window(x, bid, doc.count(d), B, w, w, groups, window, sums, out, aux, mode,
                                          _aux_graph(doc, d, how), 1e-5, 'silu', mean, mean.clone())
            finally:
                ops.AUX_PLAN = saved
        with pytest.raises(_lib.OfxError, match='invalid argument'):
            _lib.call('ofx_gn_finalize_window', _lib.ptr(sums), _lib.ptr(doc.count(d)), B, Cc, groups, window[0], window[1],
                      1e-5, 1e-5, _lib.ptr(mean), _lib.ptr(mean), _lib.stream())
    del g


@pytest.mark.parametrize('cin,cout,window', [(384, 128, (288, 384)), (256, 128, (128, 256))])
def test_split_conv_matches_the_single_call_and_the_oracle(cin, cout, window):
    """prepare_skip (planned for 8 and for 16 compute units: tiles are cut) + the late half with the time embedding, the
    partial as residual and the statistics epilogue, against the block's one-launch path and the oracle in float64."""
    from octfusion_amd import modules as M, ops
    from oracle import modules as OM
    doc, o_doc = _tree()
    d = 4
    N, B = doc.csr(d)[2], doc.batch_size
    assert 3000 <= N <= 6000 and N % 256 and N % 64
    c_h = cin - cout if cin == 384 else cin // 2
    blk = M.GraphResBlockEmbed(cin, 64, 0.0, cout, 7, 7, d - 1)
    assert M.skip_window(c_h, cin - c_h, blk.block1_norm.group) == window
    sd = C.fill_state_dict([(k, tuple(v.shape)) for k, v in blk.state_dict().items()])
    blk.load_state_dict(sd)
    blk = blk.to(dev())
    nt = d - 1
    x = C.rand_input('skipahead_x_%d' % cin, N, cin) * 1.3 + 0.2
    emb = C.rand_input('skipahead_e_%d' % cin, B, cout)
    h_ref = OM.silu(OM.dual_octree_group_norm(x.double(), o_doc, d, sd['block1_norm.weights'].double(),
                                              sd['block1_norm.bias'].double()))
    ref = OM.graph_conv(h_ref, o_doc, d, sd['conv1.weights'].double(), None, nt) + emb.double()[o_doc.batch_id(d)]
    bound = _layer_bound()
    xg, eg = x.to(dev()), emb.to(dev())
    bid = doc.batch_id32(d)
    skip_stats = ops.gn_sums(xg[:, c_h:], bid, B)
    h_stats = ops.gn_sums(xg[:, :c_h], bid, B)
    saved = ops.PLANES_MIN_TILES
    ops.PLANES_MIN_TILES = 1
    try:
        mode = blk.conv1.planes_mode(doc, d)
        assert mode == 3

        def stats_ok(y):
            st = ops.get_stats(y)
            assert st is not None
            want = torch.zeros(B, cout, 2, dtype=torch.float64, device=dev())
            want[:, :, 0].index_add_(0, bid.long(), y.double())
            want[:, :, 1].index_add_(0, bid.long(), y.double() ** 2)
            assert float((st.view(B, cout, 2) - want).abs().max()) <= 1e-5 * float(want.abs().max())

        with ops.stats_scope(dev()):
            setattr(xg, ops.STATS_ATTR, torch.cat([h_stats.view(B, c_h, 2), skip_stats.view(B, cin - c_h, 2)], 1).reshape(-1))
            hp = blk.block1_norm(xg, doc, d, act='silu', planes=mode)
            single = blk.conv1(hp, doc, d, emb=eg)
            delattr(xg, ops.STATS_ATTR)
            e1 = errors(single, ref)
            print('single', e1)
            assert e1['rel_to_max'] < bound, e1
            stats_ok(single)
            for cus in (8, 16):
                outs = []
                for rep in range(2):
                    assert blk.prepare_skip(xg, doc, d, cus, c_h=c_h, skip_stats=skip_stats)
                    assert blk.ahead_pending(xg, h_stats=h_stats)
                    y = blk._finish_ahead(xg, doc, d, eg)
                    outs.append(y)
                e2 = errors(outs[0], ref)
                d12 = float((outs[0] - single).abs().max()) / float(ref.abs().max())
                print('split, %d CUs' % cus, e2, 'vs single (rel to max)', d12)
                assert e2['rel_to_max'] < bound, (cus, e2)
                assert d12 <= 2 * bound, (cus, d12)
                stats_ok(outs[0])
                assert torch.equal(outs[0], outs[1]), 'two repeats differ'
                assert torch.equal(ops.get_stats(outs[0]), ops.get_stats(outs[1]))
        torch.cuda.synchronize()
        assert not ops.sync_error(dev())
    finally:
        ops.PLANES_MIN_TILES = saved


def test_whole_step_skip_ahead_on_off_and_graph_replay():
    """A small hr net (model_channels 64, channel_mult (1, 2, 4)) with its nested lr net on the depth-5 tree: skip-ahead
    on against off within the bound of the full-width step test, both against the oracle; captured with torch.cuda.graph
    and replayed twice, the step gives the eager result bit for bit."""
    from octfusion_amd import modules as M, ops
    from octfusion_amd.graph_unet_union import UNet3DModel
    from oracle import modules as OM, sampler as OS, unet as OU
    doc, o_doc = _tree()
    h, l = dict(C.TINY_HR_CFG, model_channels=64), C.TINY_LR_CFG
    cfg = dict(stage_flag='hr', image_size=[8, 32], input_depth=[3, 5], unet_type=['lr', 'hr'], full_depth=3,
               input_channels=[8, 3], out_channels=[8, 3], model_channels=[l['model_channels'], h['model_channels']],
               num_res_blocks=[[1, 1, 1], h['num_res_blocks']], attention_resolutions=[2, 4],
               channel_mult=[l['channel_mult'], h['channel_mult']], num_heads=4, use_checkpoint=False, dims=3)
    net = UNet3DModel(**cfg)
    sd = C.fill_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()])
    # (the zero-initialised layers would hide the decoder: conv2 of every block and the output convolution get weights)
    net.load_state_dict(sd)
    net = net.to(dev()).eval()
    B = doc.batch_size
    x = C.rand_input('skipahead_step', doc.total_num, 3)
    log_snr = OS.beta_linear_log_snr(torch.tensor([0.5, 0.3, 0.7]))
    parts = {p: OM._sub(sd, p) for p in ('unet_lr', 'unet_hr')}
    ref = OU.hr_forward(parts['unet_hr'], h, x, o_doc, log_snr, None, parts['unet_lr'], l)
    bound = FW.MODES[0][2]
    xg, tg = x.to(dev()), log_snr.to(dev())
    taken = []
    orig = M.GraphResBlockEmbed.prepare_skip

    def counting(self, *a, **k):
        r = orig(self, *a, **k)
        taken.append((self.channels, self.out_channels, r))
        return r

    def step():
        return net(unet_type='hr', x=xg, doctree=doc, unet_lr=net.unet_lr, timesteps=tg, x_self_cond=None, label=None)
    saved = (ops.SKIP_AHEAD, ops.PLANES_MIN_TILES)
    ops.PLANES_MIN_TILES = 1                 # the planes kernel on this tree's few rows
    M.GraphResBlockEmbed.prepare_skip = counting
    try:
        ops.SKIP_AHEAD = False
        off = step()
        assert not taken
        ops.SKIP_AHEAD = True
        on = step()
        split = [t for t in taken if t[2]]
        assert sorted(t[:2] for t in split) == [(128, 64), (256, 256), (384, 128)], taken
        e_off, e_on = errors(off, ref), errors(on, ref)
        d = float((on - off).abs().max()) / float(ref.abs().max())
        print('off', e_off, 'on', e_on, 'on vs off (rel to max)', d)
        assert e_off['rel_to_max'] < bound and e_on['rel_to_max'] < bound and d < bound
        assert torch.equal(on, step()), 'two eager steps differ'
        # capture on the stream the eager steps ran on (its scratch and the side stream's exist: ops._no_capture)
        s = ops.side_stream(dev())
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            eager = step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            y = step()
        for _ in range(2):
            y.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, eager), 'graph replay differs from the eager step'
        assert torch.equal(eager, on)
        assert not ops.sync_error(dev())
    finally:
        M.GraphResBlockEmbed.prepare_skip = orig
        ops.SKIP_AHEAD, ops.PLANES_MIN_TILES = saved
