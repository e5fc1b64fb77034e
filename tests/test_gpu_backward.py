"""Backward kernels at training-scale gradients, real widths and real trees.

tests/test_gpu_parity.py checks every gradient kernel on depth-5 random trees, widths <= 128 and upstream gradients
drawn from N(0, 1).  Training does not look like that: the loss gradient of an MSE over 1e5..1e7 elements starts at
2 / numel (1e-5..1e-7), the layers are 256..768 wide, and the workspace-dependent branches of the weight-gradient
entry points only run when a layer does not fit one chunk.  Three parts:

  A  gradient-scale contract: every data-gradient path (the contraction that puts dy in the activation slot of the
     fp16-pair GEMM) with dy = g * 2^-k, k in KS, judged on dx * 2^k against float64 with the bound of
     tests/test_gpu_range.py: figure <= max(3 x the figure of torch's own fp32 contraction, 2e-5), for the element-wise
     99.9th percentile and for rel-to-max.  Then the same for the whole hr / lr backward of the tiny golden nets.
  B  the chunk loop, the slice-count fallback and the OFX_EINVAL exits of ofx_graphconv_bwd_weight,
     ofx_gridconv_bwd_weight and ofx_gemm_tn_f32, reached with a deliberately small ws_bytes.
  C  GraphConv dx / dW at the configs' widths on the shell-6 / shell-8 trees (reverse segments with weights != 1), a
     batch with an empty element, GroupNorm and attention backward at real sizes, bit-for-bit determinism.

References are float64 on the CPU: closed forms over the ORACLE's edge list (dW = col_data^T dy, dx = A^T (dy W_dir^T)
with A the segment-mean matrix of oracle/modules.py graph_conv), torch conv3d autograd, the oracle's group norm.
Figures measured on an MI355X are recorded in DESIGN.md section 4.3.
"""
import functools
import math

import pytest
import torch

import common as C
from test_gpu_fullwidth import _Modes, dev, errors, report, shell6, shell8_gpu, shell8_oracle

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

KS = (0, 10, 17, 20, 23, 27)


def _within(e, floor, what):
    """The bound of tests/test_gpu_range.py, on both figures."""
    assert e['elementwise_p999'] <= max(3 * floor['elementwise_p999'], 2e-5), (what, e, floor)
    assert e['rel_to_max'] <= max(3 * floor['rel_to_max'], 2e-5), (what, e, floor)


def _scale_curve(path, g, run, ref64, ref32):
    """run(dy) -> dx on the device for dy = g * 2^-k, every k of KS; dx * 2^k against ref64 (float64 of g), with the
    floor = ref32 (torch fp32 on the CPU, scale-free) against ref64.  Returns the number of (path, k) cases run."""
    floor = errors(ref32, ref64)
    _within(floor, floor, path)
    n = 0
    for k in KS:
        dx = run((g * 2.0 ** -k).to(dev()))
        e = errors(dx.double().cpu() * 2.0 ** k, ref64)
        report(dict(test='backward_gradient_scale', path=path, k=k, precision='fp16x3', reference_fp32_noise=floor, **e))
        _within(e, floor, (path, k))
        n += 1
    return n


# ---------------------------------------------------------------------------------------------------------------
# float64 / float32 closed forms of GraphConv's gradients over the oracle's edge list
def _seg_mean_matrix(o_doc, d, N, dtype):
    """Sparse A [N * 7, N]: col_data = A @ x is oracle.modules.graph_conv's scatter_mean(x[col], row * 7 + dir)."""
    g = o_doc.graph[d]
    row, col = g['edge_idx']
    key = row * 7 + g['edge_dir']
    cnt = torch.bincount(key, minlength=N * 7)
    w = (1.0 / cnt[key].double()).to(dtype)
    return torch.sparse_coo_tensor(torch.stack([key, col]), w, (N * 7, N)).coalesce()


def _gconv_dx_ref(o_doc, d, dy, W, cin, nt, dtype):
    N, cout = dy.shape
    A = _seg_mean_matrix(o_doc, d, N, dtype)
    Wd = W.to(dtype).view(7, cin + nt, cout)[:, :cin]                  # [dir, c, o]
    G = dy.to(dtype) @ Wd.permute(2, 0, 1).reshape(cout, 7 * cin)       # [N, dir * cin + c]
    return torch.sparse.mm(A.t(), G.view(N * 7, cin))


def _gconv_dw_ref(o_doc, d, x, dy, nt, dtype):
    N = x.shape[0]
    A = _seg_mean_matrix(o_doc, d, N, dtype)
    xin = x.to(dtype)
    if nt:
        onehot = torch.nn.functional.one_hot(o_doc.graph[d]['node_type'], num_classes=nt).to(dtype)
        xin = torch.cat([xin, onehot], 1)
    col = torch.sparse.mm(A, xin).view(N, 7 * xin.shape[1])
    return col.t() @ dy.to(dtype)


def _weights(name, cin, nt, cout):
    return C.rand_input(name, 7 * (cin + nt), cout) * (1.5 / math.sqrt(7 * (cin + nt)))


@functools.lru_cache(maxsize=1)
def _small_tree():
    import test_gpu_parity as P
    from oracle import dual_octree as OD, sampler as OS
    split = C.random_split_small(3, 3, 51, p=0.45)
    oc, doc = P.small(split)
    o_doc = OD.OracleDualOctree(OS.split2octree_small(split, 5, 3))
    o_doc.post_processing_for_docnn()
    return doc, o_doc


# =============================================================================================================== A
def test_gradient_scale_graphconv():
    """ops.graphconv_backward's dx: fast (cout % 32 == 0: branch-free reverse gather + aux rows) and generic (3-channel
    dy: col rows) paths, real widths on shell-6 B = 2."""
    from octfusion_amd import ops
    oc, doc, o_oc, o_doc = shell6(2)
    n = 0
    for path, d, cin, cout in [('graphconv_fast_768_256_d5', 5, 768, 256), ('graphconv_fast_256_256_d6', 6, 256, 256),
                               ('graphconv_generic_128_3_d6', 6, 128, 3)]:
        nt = d - 1
        N = doc.csr(d)[2]
        g = C.rand_input('gs_' + path, N, cout)
        W = _weights('gsw_' + path, cin, nt, cout)
        x = torch.zeros(N, cin, device=dev())                          # dx does not depend on x
        Wg = W.to(dev())
        ref64 = _gconv_dx_ref(o_doc, d, g, W, cin, nt, torch.float64)
        ref32 = _gconv_dx_ref(o_doc, d, g, W, cin, nt, torch.float32)
        n += _scale_curve(path, g, lambda dy: ops.graphconv_backward(x, dy, doc, d, Wg, nt, need_dw=False)[0], ref64, ref32)
    assert n == 3 * len(KS)


def test_gradient_scale_gridconv():
    """backward.gridconv_backward's dx: stride 1, stride 2 and nearest-upsample + conv, 128 -> 128 around 16^3."""
    import torch.nn.functional as F
    from octfusion_amd import backward as BW, graph_unet_lr as LR, ops
    n = 0
    for path, mode, d in [('gridconv_stride1_128_16^3', 0, 4), ('gridconv_stride2_128_16^3', 1, 4),
                          ('gridconv_upsample_128_8^3', 2, 3)]:
        B, cin, cout = 1, 128, 128
        m = LR.GridConv3d(cin, cout, mode)
        sd = C.fill_state_dict([(k, tuple(v.shape)) for k, v in m.state_dict().items()])
        m.load_state_dict(sd)
        m = m.to(dev())
        S, So = 1 << d, 1 << m.out_depth(d)
        g = C.rand_input('gs_' + path, B, cout, So, So, So)

        def ref(dtype):
            with torch.enable_grad():
                x = torch.zeros(B, cin, S, S, S, dtype=dtype, requires_grad=True)
                w = sd['weight'].to(dtype)
                if mode == 0:
                    y = F.conv3d(x, w, None, padding=1)
                elif mode == 1:
                    y = F.conv3d(x, w, None, stride=2, padding=1)
                else:
                    y = F.conv3d(F.interpolate(x, scale_factor=2, mode='nearest'), w, None, padding=1)
                (y * g.to(dtype)).sum().backward()
            return x.grad
        gs = LR.GridState(B, d, dev())
        x_rows = torch.zeros(B * 8 ** d, cin, device=dev())

        g_rows = ops.voxel2octree_cf(g.to(dev()).contiguous(), m.out_depth(d)).cpu()
        n += _scale_curve(path, g_rows, lambda dy: ops.octree2voxel_cf(BW.gridconv_backward(m, x_rows, dy, gs)[0], B, d),
                          ref(torch.float64), ref(torch.float32))
    assert n == 3 * len(KS)


def test_gradient_scale_dense_and_pool():
    """ops.linear_backward (1x1 skip convolutions, embedding linears) and the pooled GEMMs of graph down / up-sampling
    (backward._pool_bwd / _unpool_bwd), C = 256 at depth 6 <-> 5 of shell-6 B = 2."""
    from octfusion_amd import backward as BW, modules as M, ops
    n = 0
    # ---- linear: y = x W^T, dx = dy W; also the CPU-side check that the fp32 reference is scale-free at every k
    rows, cin, cout = 8192, 768, 256
    g = C.rand_input('gs_linear', rows, cout)
    W = C.rand_input('gsw_linear', cout, cin) * (1.5 / math.sqrt(cin))
    ref64 = g.double() @ W.double()
    floor = errors(g @ W, ref64)
    for k in KS:
        _within(errors(((g * 2.0 ** -k) @ W).double() * 2.0 ** k, ref64), floor, ('fp32 reference', k))
    xg, Wg = torch.zeros(rows, cin, device=dev()), W.to(dev())
    n += _scale_curve('linear_768_256', g, lambda dy: ops.linear_backward(xg, dy, Wg)[0], ref64, g @ W)
    # ---- pool / unpool
    oc, doc, o_oc, o_doc = shell6(2)
    Cc, d = 256, 6
    # pool: rows of depth 6 -> depth 5
    copy_src, gemm_rows, n_out = doc.pool_maps(d)
    numd = int(doc.nnum[d])
    Nd = doc.csr(d)[2]
    down = M.Downsample(Cc)
    wd = C.rand_input('gsw_pool', Cc, Cc, 8) * (1.5 / math.sqrt(8 * Cc))
    down.load_state_dict({'weights': wd})
    down = down.to(dev())
    g = C.rand_input('gs_pool', n_out, Cc)
    cs, gr = copy_src.cpu().long(), gemm_rows.cpu().long()

    def pool_ref(dtype):
        dx = torch.zeros(Nd, Cc, dtype=dtype)
        keep = cs >= 0
        dx[cs[keep]] = g.to(dtype)[:cs.numel()][keep]
        dx[Nd - numd:] = (g.to(dtype)[gr] @ wd.to(dtype).view(Cc, 8 * Cc)).view(numd, Cc)
        return dx
    assert gr.numel() * 8 == numd and gr.numel() > 1000
    xz = torch.zeros(Nd, Cc, device=dev())
    n += _scale_curve('pool_256_d6', g, lambda dy: BW._pool_bwd(down, xz, dy, doc, d, BW._Grads(), 'p.'),
                      pool_ref(torch.float64), pool_ref(torch.float32))
    # unpool: rows of depth 5 -> depth 6
    d = 5
    copy_src, a_rows, n_copy = doc.unpool_maps(d)
    N5 = doc.csr(d)[2]
    n_ne = a_rows.numel()
    up = M.Upsample(Cc)
    wu = C.rand_input('gsw_unpool', Cc, Cc, 8) * (1.5 / math.sqrt(Cc))
    up.load_state_dict({'weights': wu})
    up = up.to(dev())
    g = C.rand_input('gs_unpool', n_copy + 8 * n_ne, Cc)
    cs, ar = copy_src.cpu().long(), a_rows.cpu().long()

    def unpool_ref(dtype):
        dx = torch.zeros(N5, Cc, dtype=dtype)
        dx[cs] = g.to(dtype)[:n_copy]
        dx[ar] = g.to(dtype)[n_copy:].reshape(n_ne, 8 * Cc) @ wu.to(dtype).view(Cc, 8 * Cc).t()
        return dx
    assert n_ne > 1000
    xz5 = torch.zeros(N5, Cc, device=dev())
    n += _scale_curve('unpool_256_d5', g, lambda dy: BW._unpool_bwd(up, xz5, dy, doc, d, BW._Grads(), 'u.'),
                      unpool_ref(torch.float64), unpool_ref(torch.float32))
    assert n == 3 * len(KS)


def _grads_close(got, ref, k):
    """The tolerance of test_lr / test_hr_unet_backward_vs_autograd (tests/test_gpu_parity.py), between the gradients
    of a loss gradient scaled by 2^-k (scaled back) and the unscaled ones."""
    assert set(got) == set(ref)
    gmax = max(float(v.abs().max()) for v in ref.values())
    for name in ref:
        r = ref[name]
        err = float((got[name] * 2.0 ** k - r).abs().max())
        assert err <= 5e-3 * float(r.abs().max()) + 2e-5 * gmax, (name, k, err, float(r.abs().max()), gmax)
    return len(ref)


def test_gradient_scale_whole_steps(golden):
    """The backward of training.hr_stage_step / lr_stage_step (backward.hr_ / lr_unet_forward_backward with the MSE's
    dy = 2 diff / numel) for the tiny golden nets, the loss gradient multiplied by 2^-k: every gradient equals 2^-k
    times the unscaled one.  k = 12 puts the tiny nets (numel ~ 1e4) where the bench sizes are (numel ~ 1e6..1e7)."""
    import test_gpu_parity as P
    from octfusion_amd import backward as BW, graph_unet_lr as LR, graph_unet_union as U, ops
    ks = (12, 20)
    # ---- hr stage (nested lr net)
    G = golden('g_unet')
    r = G['uncond']
    oc, doc = P.small(G['split_small'])
    net = P.load(U.UNet3DModel(**P.union_cfg(None)), r['keys'])
    N = doc.total_num
    x = C.rand_input('hrb_x', N, 3).to(dev())
    target = C.rand_input('hrb_dy', N, 3).to(dev())
    t = torch.tensor([0.4, -0.9]).to(dev())

    def hr(k):
        _, dx, g_hr, g_lr = BW.hr_unet_forward_backward(
            net.unet_hr, x, doc, net.unet_lr, t, lambda y: (y - target) * (2.0 / y.numel()) * 2.0 ** -k)
        out = {'unet_hr.' + n_: v for n_, v in g_hr.items()}
        out.update({'unet_lr.' + n_: v for n_, v in g_lr.items()})
        out['dx'] = dx
        return out
    ref = hr(0)
    n = sum(_grads_close(hr(k), ref, k) for k in ks)
    assert n == len(ks) * len(ref) and len(ref) > 100
    # ---- lr stage
    keys = golden('g_dense')['lr']['keys']
    lnet = P.load(LR.UNet3DModel(**C.TINY_LR_CFG), keys)
    B, S = 2, 8
    rows = ops.voxel2octree_cf(C.rand_input('lrb_x', B, 16, S, S, S).to(dev()), 3)
    tgt = ops.voxel2octree_cf(C.rand_input('lrb_dy', B, 8, S, S, S).to(dev()), 3)
    tl = torch.tensor([0.3, -1.2]).to(dev())

    def lr(k):
        _, dx, g = BW.lr_unet_forward_backward(lnet, rows, B, tl, lambda y: (y - tgt) * (2.0 / y.numel()) * 2.0 ** -k)
        g = dict(g)
        g['dx'] = dx
        return g
    ref = lr(0)
    n = sum(_grads_close(lr(k), ref, k) for k in ks)
    assert n == len(ks) * len(ref) and len(ref) > 50


# =============================================================================================================== B
def _cdiv(a, b):
    return (a + b - 1) // b


def _generic_ws_bytes(Kp, cout, chunk):
    """ws_bytes that makes the generic (col rows) path of the two conv weight gradients take `chunk` rows at a time:
    the partial sums come first (slices = min(64, ceil(512 / tiles)), 256-byte aligned), the col rows after them."""
    tiles = _cdiv(Kp, 128) * _cdiv(cout, 128)
    slices = min(64, _cdiv(512, tiles))
    part = (slices * Kp * cout * 4 + 255) // 256 * 256
    return part, part + chunk * Kp * 4 + 64


def _gconv_dw_call(doc, d, x, dy, cin, nt, ws, ws_bytes, fast, out=None):
    """ofx_graphconv_bwd_weight through the C ABI with an explicit ws_bytes; returns dW in the reference's row order."""
    from octfusion_amd import _lib
    from octfusion_amd._lib import call, ptr, stream
    N, cout = dy.shape
    seg_ptr, col, Ng, E = doc.csr(d)
    assert N == Ng
    Kp = _lib.lib().ofx_graphconv_packed_k(cin, nt)
    ntp = (7 * nt + 31) // 32 * 32 if nt else 0
    Kf = Kp - ntp
    tf = doc.type_frac(d, nt) if nt else None
    nbr_ext, multi_seg, V = doc.ext(d)
    aux = torch.empty((V + 1) * cin, dtype=torch.float32, device=x.device) if fast else None
    dwp = out if out is not None else torch.empty(Kp, cout, dtype=torch.float32, device=x.device)
    call('ofx_graphconv_bwd_weight', ptr(x), x.stride(0), cin, N, ptr(doc.nbr(d)), ptr(seg_ptr), ptr(col),
         ptr(nbr_ext) if fast else None, ptr(multi_seg) if fast else None, V if fast else 0, ptr(aux),
         ptr(tf), tf.stride(0) if nt else 0, tf.shape[1] if nt else 0, ptr(dy), dy.stride(0), cout, ptr(dwp), Kp,
         ptr(ws), ws_bytes, stream())
    dirs = torch.arange(7, device=x.device).view(7, 1)
    idx = [dirs * cin + torch.arange(cin, device=x.device).view(1, cin)]
    if nt:
        idx.append(Kf + dirs * nt + torch.arange(nt, device=x.device).view(1, nt))
    return dwp.index_select(0, torch.cat(idx, 1).reshape(-1))


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def _both_precisions(run, ref64, what):
    """run() in the default precision (5e-5 rel-to-max, bf16-pair TN contraction) and in exact fp32 (1e-5)."""
    from octfusion_amd import ops
    out = []
    for prec, tol in ((ops.DEFAULT_PRECISION, 5e-5), ('fp32', 1e-5)):
        with _Modes(prec, True):
            got = run()
        e = _rel(got, ref64)
        assert e <= tol, (what, prec, e)
        out.append(got)
    return out


def test_graphconv_weight_gradient_chunks_and_small_workspaces():
    from octfusion_amd import _lib, ops
    doc, o_doc = _small_tree()
    d = 5
    N = doc.csr(d)[2]
    assert N % 32 != 0 and N > 2200
    ws = ops.workspace(dev())
    cases = 0
    for cin, nt, cout in [(3, 0, 64), (3, 4, 36), (24, 0, 36), (24, 4, 64)]:
        x = C.rand_input('wsx%d_%d' % (cin, nt), N, cin)
        dy = C.rand_input('wsdy%d_%d' % (cin, cout), N, cout)
        ref = _gconv_dw_ref(o_doc, d, x, dy, nt, torch.float64)
        xg, dyg = x.to(dev()), dy.to(dev())
        Kp = _lib.lib().ofx_graphconv_packed_k(cin, nt)
        chunk = N // 3 // 32 * 32                                          # three full chunks and a ragged one
        part, small = _generic_ws_bytes(Kp, cout, chunk)
        nchunks = _cdiv(N, chunk)
        assert nchunks >= 3 and (N - (nchunks - 1) * chunk) % 32 != 0
        big = _both_precisions(lambda: _gconv_dw_call(doc, d, xg, dyg, cin, nt, ws, ws.numel(), False), ref, (cin, nt, 'big'))
        chunked = _both_precisions(lambda: _gconv_dw_call(doc, d, xg, dyg, cin, nt, ws, small, False), ref, (cin, nt, 'chunked'))
        one = _both_precisions(lambda: _gconv_dw_call(doc, d, xg, dyg, cin, nt, ws, _generic_ws_bytes(Kp, cout, 32)[1], False),
                               ref, (cin, nt, '32-row chunks'))
        for b, c_, o, tol in zip(big, chunked, one, (5e-5, 1e-5)):
            assert _rel(c_, b) <= tol and _rel(o, b) <= tol
        # too small for one 32-row chunk, and too small for the partial sums: OFX_EINVAL, nothing written
        for bad in (part + 31 * Kp * 4, part, 1024):
            sentinel = torch.full((Kp, cout), 7.0, device=dev())
            with pytest.raises(_lib.OfxError, match='ofx_graphconv_bwd_weight'):
                _gconv_dw_call(doc, d, xg, dyg, cin, nt, ws, bad, False, out=sentinel)
            torch.cuda.synchronize()
            assert bool((sentinel == 7.0).all())
        cases += 1
    # fast path (cin % 32 == 0): the slice count falls to what the workspace holds, down to one slice
    for cin, nt, cout in [(64, 4, 96), (32, 0, 132)]:
        x = C.rand_input('wsx%d_%d' % (cin, nt), N, cin)
        dy = C.rand_input('wsdy%d_%d' % (cin, cout), N, cout)
        ref = _gconv_dw_ref(o_doc, d, x, dy, nt, torch.float64)
        xg, dyg = x.to(dev()), dy.to(dev())
        Kp = _lib.lib().ofx_graphconv_packed_k(cin, nt)
        total = Kp * cout * 4
        big = _both_precisions(lambda: _gconv_dw_call(doc, d, xg, dyg, cin, nt, ws, ws.numel(), True), ref, (cin, 'big'))
        for nbytes in (total, 3 * total + 100):
            got = _both_precisions(lambda: _gconv_dw_call(doc, d, xg, dyg, cin, nt, ws, nbytes, True), ref, (cin, nbytes))
            for b, g_, tol in zip(big, got, (5e-5, 1e-5)):
                assert _rel(g_, b) <= tol
        sentinel = torch.full((Kp, cout), 7.0, device=dev())
        with pytest.raises(_lib.OfxError, match='ofx_graphconv_bwd_weight'):
            _gconv_dw_call(doc, d, xg, dyg, cin, nt, ws, total - 16, True, out=sentinel)
        torch.cuda.synchronize()
        assert bool((sentinel == 7.0).all())
        cases += 1
    # n_nodes = 0 zero-fills dWp
    from octfusion_amd._lib import call, ptr, stream
    dwp = torch.full((32, 64), 7.0, device=dev())
    call('ofx_graphconv_bwd_weight', None, 4, 3, 0, None, None, None, None, None, 0, None, None, 0, 0, ptr(dwp), 64, 64,
         ptr(dwp), 32, ptr(ws), ws.numel(), stream())
    assert bool((dwp == 0).all())
    assert cases == 6


def test_gridconv_weight_gradient_chunks_and_small_workspaces():
    import torch.nn.functional as F
    from octfusion_amd import _lib, graph_unet_lr as LR, ops
    from octfusion_amd._lib import call, ptr, stream
    ws = ops.workspace(dev())
    cases = 0
    for B, d, cin, cout, fast in [(3, 3, 16, 64, False), (3, 3, 32, 36, True)]:
        S = 1 << d
        n = B * 8 ** d
        x = C.rand_input('gwx%d' % cin, B, cin, S, S, S)
        dy = C.rand_input('gwdy%d' % cout, B, cout, S, S, S)
        with torch.enable_grad():
            w64 = torch.zeros(cout, cin, 3, 3, 3, dtype=torch.float64, requires_grad=True)
            (F.conv3d(x.double(), w64, None, padding=1) * dy.double()).sum().backward()
        ref = w64.grad
        gs = LR.GridState(B, d, dev())
        xr = ops.voxel2octree_cf(x.to(dev()).contiguous(), d)
        dyr = ops.voxel2octree_cf(dy.to(dev()).contiguous(), d)
        Kp = _lib.lib().ofx_conv3d_packed_k(cin)

        def run(nbytes, out=None):
            dwp = out if out is not None else torch.empty(Kp, cout, dtype=torch.float32, device=dev())
            call('ofx_gridconv_bwd_weight', ptr(xr), xr.stride(0), cin, n, n,
                 None if fast else ptr(gs.cache.table(0, d, False)), ptr(gs.cache.table(0, d, True)) if fast else None,
                 ptr(ops.zero_row(dev())) if fast else None, ptr(dyr), dyr.stride(0), cout, ptr(dwp), ptr(ws), nbytes,
                 stream())
            return dwp[:27 * cin].view(27, cin, cout).permute(2, 1, 0).reshape(cout, cin, 3, 3, 3)
        big = _both_precisions(lambda: run(ws.numel()), ref, (cin, 'big'))
        if fast:
            total = Kp * cout * 4
            sizes, bad = (total, 2 * total + 48), (total - 16,)
        else:
            chunk = 32 * 17                                               # 1536 rows: 2 full chunks + 448 -> 3 chunks;
            part, small = _generic_ws_bytes(Kp, cout, chunk)              # 544-row chunks split into 64 slices of 32
            assert _cdiv(n, chunk) >= 3 and n % chunk != 0
            sizes, bad = (small, _generic_ws_bytes(Kp, cout, 32)[1]), (part + 31 * Kp * 4, part)
        for nbytes in sizes:
            got = _both_precisions(lambda: run(nbytes), ref, (cin, nbytes))
            for b, g_, tol in zip(big, got, (5e-5, 1e-5)):
                assert _rel(g_, b) <= tol
        for nbytes in bad:
            sentinel = torch.full((Kp, cout), 7.0, device=dev())
            with pytest.raises(_lib.OfxError, match='ofx_gridconv_bwd_weight'):
                run(nbytes, out=sentinel)
            torch.cuda.synchronize()
            assert bool((sentinel == 7.0).all())
        cases += 1
    assert cases == 2


def test_gemm_tn_rows_strides_and_small_workspaces():
    from octfusion_amd import _lib, ops
    from octfusion_amd._lib import call, ptr, stream
    ws = ops.workspace(dev())
    cases = 0
    for rows in (1, 31, 33, 32 * 256 + 1, 100003):
        for K, N in ((64, 128), (132, 4)):
            gen = torch.Generator().manual_seed(rows + K)
            Pb = torch.randn(rows, K + 12, generator=gen)                 # ldp = K + 12, ldq = N + 4: not contiguous
            Qb = torch.randn(rows, N + 4, generator=gen)
            ref = Pb[:, :K].double().t() @ Qb[:, :N].double()
            Pg, Qg = Pb.to(dev()), Qb.to(dev())

            def run(nbytes, out=None):
                o = out if out is not None else torch.empty(K, N, dtype=torch.float32, device=dev())
                call('ofx_gemm_tn_f32', ptr(Pg), Pg.stride(0), ptr(Qg), Qg.stride(0), rows, K, N, ptr(o), ptr(ws), nbytes,
                     stream())
                return o
            total = K * N * 4
            big = _both_precisions(lambda: run(ws.numel()), ref, (rows, K, 'big'))
            # the workspace loop: down to 1 and to 2 slices.  One slice is one sequential fp32 accumulation over all
            # the rows, whose own rounding (~ 2^-24 sqrt(rows) against float64) reaches the 1e-5 bound of the exact-fp32
            # mode at 1e5 rows (measured 1.15e-5): the 100 003-row case goes down to 16 and 17 slices instead
            few = 1 if rows <= 32 * 256 + 1 else 16
            for nbytes in (few * total, (few + 1) * total + 16):
                got = _both_precisions(lambda: run(nbytes), ref, (rows, K, nbytes))
                for b, g_, tol in zip(big, got, (5e-5, 1e-5)):
                    assert _rel(g_, b) <= tol
            sentinel = torch.full((K, N), 7.0, device=dev())
            with pytest.raises(_lib.OfxError, match='ofx_gemm_tn_f32'):
                run(total - 16, out=sentinel)
            torch.cuda.synchronize()
            assert bool((sentinel == 7.0).all())
            cases += 1
    out = torch.full((8, 4), 7.0, device=dev())
    call('ofx_gemm_tn_f32', None, 8, None, 4, 0, 8, 4, ptr(out), ptr(ws), ws.numel(), stream())
    assert bool((out == 0).all())
    assert cases == 10


def _col_ws_cases(name, run, ref64, out_shape, Kp, ws):
    """The workspace contract of the col path (include/ofx.h): run(ws, ws_bytes, out) with (i) the full workspace and
    (ii) exactly the documented sufficient 588 * Kp bytes matches float64; (iii) no workspace and (iv) 128 col rows
    without their tail are OFX_EINVAL argument checks that leave `out` alone."""
    from octfusion_amd import _lib
    for nbytes in (ws.numel(), 588 * Kp):
        out = torch.full(out_shape, 7.0, device=dev())
        run(ws, nbytes, out)
        e = _rel(out, ref64)
        report(dict(test='col_path_workspace', path=name, ws_bytes=nbytes, rel_to_max=e))
        assert e <= 5e-5, (name, nbytes, e)
    for w, nbytes in ((None, 0), (None, ws.numel()), (ws, 512 * Kp)):
        out = torch.full(out_shape, 7.0, device=dev())
        with pytest.raises(_lib.OfxError, match=name.split(' ')[0]):
            run(w, nbytes, out)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), (name, nbytes)


def test_col_path_workspace_contract():
    """ofx_graphconv_fwd, ofx_graphconv_bwd_data and ofx_gridconv_fwd on layers the branch-free kernel cannot take:
    the workspace is required (there is no in-kernel gather behind it), 588 * Kp bytes are enough, and the table path
    (cin % 32 == 0 with nbr_ext) still needs none."""
    import torch.nn.functional as F
    from octfusion_amd import _lib, graph_unet_lr as LR, ops
    from octfusion_amd._lib import call, ptr, stream
    doc, o_doc = _small_tree()
    d = 4
    seg_ptr, col, N, E = doc.csr(d)
    assert N > 256 and N % 128 != 0                                        # many 128-row chunks and a ragged one
    ws = ops.workspace(dev())
    cout = 32
    A = _seg_mean_matrix(o_doc, d, N, torch.float64)
    nbr_ext, multi_seg, V = doc.ext(d)

    def fwd(x, pw, cin, table, w, nbytes, out):
        aux = torch.empty((V + 1) * cin, dtype=torch.float32, device=dev()) if table else None
        call('ofx_graphconv_fwd', ptr(x), cin, cin, N, ptr(doc.nbr(d)), ptr(seg_ptr), ptr(col),
             ptr(nbr_ext) if table else None, ptr(multi_seg) if table else None, V if table else 0, ptr(aux), None, 0, 0,
             ptr(pw.t), pw.Kp, cout, None, None, 0, None, None, 0, ptr(out), cout, None, cout, ptr(w), nbytes, stream())

    for cin in (3, 24, 64):
        x = C.rand_input('cwx%d' % cin, N, cin)
        W = _weights('cww%d' % cin, cin, 0, cout)
        ref = torch.sparse.mm(A, x.double()).view(N, 7 * cin) @ W.double()
        xg = x.to(dev())
        pw = ops.PackedWeight().get(W.to(dev()), 'graphconv', cin, 0)
        if cin == 64:                                                      # table path: never needed the workspace
            out = torch.full((N, cout), 7.0, device=dev())
            fwd(xg, pw, cin, True, None, 0, out)
            assert _rel(out, ref) <= 5e-5
        else:
            _col_ws_cases('ofx_graphconv_fwd cin=%d' % cin, lambda w, nb, out: fwd(xg, pw, cin, False, w, nb, out), ref,
                          (N, cout), pw.Kp, ws)

    # dx of the same layers: the gathered operand is dy.  No reverse table for the layers of the forward cases; with
    # one, a dy of 24 channels still takes the col path
    rv = doc.rev(d)
    for cin, co, table in ((3, 32, False), (24, 32, False), (32, 24, True)):
        dy = C.rand_input('cwdy%d_%d' % (cin, co), N, co)
        W = _weights('cwbw%d_%d' % (cin, co), cin, 0, co)
        ref = _gconv_dx_ref(o_doc, d, dy, W, cin, 0, torch.float64)
        dyg = dy.to(dev())
        wt = W.view(7, cin, co).permute(0, 2, 1).reshape(7 * co, cin).contiguous().to(dev())
        pwt = ops.PackedWeight().get(wt, 'graphconv', co, 0)

        def bwd(w, nbytes, out, dyg=dyg, pwt=pwt, cin=cin, co=co, table=table):
            call('ofx_graphconv_bwd_data', ptr(dyg), co, co, N, ptr(rv['nbr']), ptr(rv['rev_ptr']), ptr(rv['rev_row']),
                 ptr(rv['rev_w']), ptr(rv['nbr_ext']) if table else None, ptr(rv['multi_seg']) if table else None,
                 rv['V'] if table else 0, None, ptr(pwt.t), pwt.Kp, cin, ptr(out), cin, ptr(w), nbytes, stream())
        _col_ws_cases('ofx_graphconv_bwd_data cin=%d cout=%d' % (cin, co), bwd, ref, (N, cin), pwt.Kp, ws)

    # 4^3 grid, 3 -> 32 channels
    B, gd, cin = 3, 2, 3
    S, n = 1 << gd, B * 8 ** gd
    x = C.rand_input('cwgx', B, cin, S, S, S)
    wgt = C.rand_input('cwgw', cout, cin, 3, 3, 3) * (1.5 / math.sqrt(27 * cin))
    ref = F.conv3d(x.double(), wgt.double(), None, padding=1)
    gs = LR.GridState(B, gd, dev())
    xr = ops.voxel2octree_cf(x.to(dev()).contiguous(), gd)
    pc = ops.PackedConv3d().get(wgt.to(dev()))
    Kp = _lib.lib().ofx_conv3d_packed_k(cin)

    def grid(w, nbytes, out):
        call('ofx_gridconv_fwd', ptr(xr), xr.stride(0), cin, n, n, ptr(gs.cache.table(0, gd, False)), None,
             ptr(ops.zero_row(dev())), ptr(pc.t), cout, None, None, 0, None, None, 0, ptr(out), cout, ptr(w), nbytes,
             stream())
    # (the float64 oracle rounded to fp32 on its way through the row layout: 2^-24, far below the bound)
    _col_ws_cases('ofx_gridconv_fwd cin=3', grid, ops.voxel2octree_cf(ref.float().to(dev()).contiguous(), gd), (n, cout), Kp, ws)


# =============================================================================================================== C
def _check_reverse_tables(doc, o_doc, d):
    """doc.rev(d) against the host construction of test_graphconv_backward_vs_autograd; returns (non-empty reverse
    segments, those with several entries, those carrying a weight != 1).

    The two kinds never coincide on a dual octree graph: a coarse leaf that faces four finer nodes has ONE forward
    segment of four entries (each finer node's reverse segment then holds that single edge with weight 1/4), while
    each of the four finer nodes names the leaf alone (the leaf's reverse segment holds four edges of weight 1).
    Both kinds go through the weighted aux rows of multi_mean_kernel, so both are required."""
    g = o_doc.graph[d]
    row, col = g['edge_idx']
    key = row * 7 + g['edge_dir']
    cnt = torch.bincount(key, minlength=int(key.max()) + 1)[key].float()
    rkey = col * 7 + g['edge_dir']
    order = torch.argsort(rkey * (int(row.max()) + 1) + row)
    rv = doc.rev(d)
    n7 = doc.csr(d)[2] * 7
    per_seg = torch.bincount(rkey, minlength=n7)
    assert torch.equal(rv['rev_ptr'].cpu().long(), torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(per_seg, 0)]))
    assert torch.equal(rv['rev_row'].cpu().long(), row[order])
    assert torch.equal(rv['rev_w'].cpu(), (1.0 / cnt)[order])
    has_frac = torch.zeros(n7, dtype=torch.long).index_add_(0, rkey, (cnt != 1).long()) > 0
    # every such segment must be served by an aux row of the branch-free gather
    assert rv['V'] == int(((per_seg > 1) | has_frac).sum())
    return torch.tensor([int((per_seg > 0).sum()), int((per_seg > 1).sum()), int(has_frac.sum())])


def _layer(doc, o_doc, d, cin, cout, nt, tag, sample=None):
    """dx and dW of one GraphConv layer against float64, both run twice (determinism).  Returns 1."""
    from octfusion_amd import ops
    N = doc.csr(d)[2]
    x = C.rand_input('cx_%s' % tag, N, cin)
    dy = C.rand_input('cdy_%s' % tag, N, cout)
    W = _weights('cw_%s' % tag, cin, nt, cout)
    xg, dyg, Wg = x.to(dev()), dy.to(dev()), W.to(dev())
    dx, dW = ops.graphconv_backward(xg, dyg, doc, d, Wg, nt)
    dx2, dW2 = ops.graphconv_backward(xg, dyg, doc, d, Wg, nt)
    assert torch.equal(dW, dW2), 'dW is not deterministic'
    assert torch.equal(dx, dx2), 'dx is not deterministic'
    dx64 = _gconv_dx_ref(o_doc, d, dy, W, cin, nt, torch.float64)
    dx32 = _gconv_dx_ref(o_doc, d, dy, W, cin, nt, torch.float32)
    dxc = dx.cpu()
    if sample is not None:
        rows = torch.randperm(N, generator=torch.Generator().manual_seed(8))[:sample]
        dxc, dx64, dx32 = dxc[rows], dx64[rows], dx32[rows]
    floor, e = errors(dx32, dx64), errors(dxc, dx64)
    dw64 = _gconv_dw_ref(o_doc, d, x, dy, nt, torch.float64)
    ew = errors(dW, dw64)
    report(dict(test='backward_fullwidth_graphconv', layer=tag, depth=d, cin=cin, cout=cout, rows=N, dx=e,
                dx_reference_fp32_noise=floor, dW=ew))
    _within(e, floor, ('dx', tag))
    assert ew['rel_to_max'] <= 5e-5, ('dW', tag, ew)
    return 1


PAIRS = [(768, 256), (512, 512), (256, 256), (128, 128), (3, 128), (128, 3)]


def test_fullwidth_graphconv_backward_shell6():
    oc, doc, o_oc, o_doc = shell6(2)
    nonempty, multi, weighted = sum(_check_reverse_tables(doc, o_doc, d) for d in (4, 5, 6)).tolist()
    # the condition that makes this test worth its name: reverse segments that sum several rows, and weights != 1
    assert multi >= 0.01 * nonempty and weighted >= 0.01 * nonempty, (nonempty, multi, weighted)
    n = 0
    for d in (4, 5, 6):
        for cin, cout in PAIRS:
            n += _layer(doc, o_doc, d, cin, cout, d - 1, 's6_d%d_%d_%d' % (d, cin, cout))
    assert n == 3 * len(PAIRS)


def test_fullwidth_graphconv_backward_shell8():
    """One depth-8 layer (448 232 rows, 64 -> 64, 7 node types): dx on 50 000 sampled rows, the whole dW."""
    doc = shell8_gpu()
    _, o_doc = shell8_oracle()
    nonempty, multi, weighted = _check_reverse_tables(doc, o_doc, 8).tolist()
    assert multi >= 0.01 * nonempty and weighted >= 0.01 * nonempty, (nonempty, multi, weighted)
    assert _layer(doc, o_doc, 8, 64, 64, 7, 's8_d8_64_64', sample=50000) == 1


def test_graphconv_backward_with_an_empty_batch_element():
    """A batch whose middle element has no node below the full layer (split[1] = -1): row ranges of the elements
    around it, and the reverse graph, must still line up."""
    import test_gpu_parity as P
    from oracle import dual_octree as OD, sampler as OS
    split = C.random_split_small(3, 3, 57, p=0.45)
    split[1] = -1.0
    oc, doc = P.small(split)
    o_doc = OD.OracleDualOctree(OS.split2octree_small(split, 5, 3))
    o_doc.post_processing_for_docnn()
    n = 0
    for d in (4, 5):
        bid = o_doc.batch_id(d)
        assert int((bid == 0).sum()) > 0 and int((bid == 2).sum()) > 0
        assert int((bid == 1).sum()) < min(int((bid == 0).sum()), int((bid == 2).sum()))
        _check_reverse_tables(doc, o_doc, d)
        for cin, cout in [(256, 256), (128, 3), (3, 128)]:
            n += _layer(doc, o_doc, d, cin, cout, d - 1, 'empty_d%d_%d_%d' % (d, cin, cout))
    assert n == 6


@functools.lru_cache(maxsize=None)
def _deep_oracle_case(kind, cin, cout, nt):
    """float64 oracle of one GraphConv layer on a deep tree of tests/graph_oracle.py, depth 6: forward, and dx / dW by
    torch.autograd of oracle.modules.graph_conv -- once per case, shared by the launches below."""
    import graph_oracle as G
    from oracle import modules as OM
    o_doc = G.tree(kind)[1]
    d = o_doc.depth
    N = int(o_doc.graph[d]['node_type'].shape[0])
    tag = '%s_%d_%d' % (kind, cin, cout)
    x = C.rand_input('dx_%s' % tag, N, cin)
    dy = C.rand_input('ddy_%s' % tag, N, cout)
    W = _weights('dw_%s' % tag, cin, nt, cout)
    with torch.enable_grad():
        x64 = x.double().requires_grad_(True)
        W64 = W.double().requires_grad_(True)
        y = OM.graph_conv(x64, o_doc, d, W64, None, nt)
        (y * dy.double()).sum().backward()
    return dict(x=x, dy=dy, W=W, ref=y.detach(), dx=x64.grad, dW=W64.grad, d=d, N=N)


@pytest.mark.parametrize('kind', ['deep_a', 'full_face'])
@pytest.mark.parametrize('cin,cout', [(32, 64), (96, 128)])
def test_graphconv_on_deep_trees(kind, cin, cout):
    """Every GraphConv launch on trees four levels deeper than their full layer (`deep_a`: segments of up to 91 rows
    over many blocks; `full_face`: nine segments of 256 rows), depth 6, against oracle.modules.graph_conv in float64:
    ofx_graphconv_fwd by its col path (no gather table) and its fast path, the planes kernel as persistent stream-K
    launch and as one tile per block, and ops.graphconv_backward's dx / dW against the oracle's autograd, run twice
    (determinism).  Bounds: the ones this file and tests/test_gpu_persistent.py use for the same entry points in the
    default precision -- dx as `_layer` judges it: against the figure of torch's own fp32 contraction on the CPU
    (`_within`), dW 5e-5."""
    import graph_oracle as G
    from octfusion_amd import _lib, modules as M, octree as PO, ops
    from octfusion_amd.dual_octree import DualOctree
    nt = 5
    K = _deep_oracle_case(kind, cin, cout, nt)
    d, N = K['d'], K['N']
    doc = DualOctree(G.build_tree(kind, PO, dev()))
    seg_ptr, col, n_rows, _ = doc.csr(d)
    assert n_rows == N and doc.max_seg(d) == (256 if kind == 'full_face' else 91)
    assert ops.get_precision() == ops.DEFAULT_PRECISION
    xg, dyg, Wg = K['x'].to(dev()), K['dy'].to(dev()), K['W'].to(dev())
    # ofx_graphconv_fwd: col path (no table), fast path (branch-free gather through nbr_ext + aux rows)
    pw = ops.PackedWeight().get(Wg, 'graphconv', cin, nt)
    tf = doc.type_frac(d, nt)
    for path, ext in (('col', None), ('fast', doc.ext(d))):
        y = ops.graphconv(xg, doc.nbr(d), seg_ptr, col, pw, cin, tf, ext=ext)
        e = _rel(y, K['ref'])
        print('ofx_graphconv_fwd', kind, cin, cout, path, e)
        assert e <= 5e-5, (path, e)
    # the planes kernel through the module, both launch shapes
    conv = M.GraphConv(cin, cout, 7, 7, nt)
    conv.load_state_dict({'weights': K['W']})
    conv = conv.to(dev())
    saved = ops.PLANES_MIN_TILES
    ops.PLANES_MIN_TILES = 1
    try:
        for persistent in (1, 0):
            _lib.call('ofx_set_gconv_persistent', persistent)
            xp = ops.planes_split(xg, conv.planes_mode(doc, d))
            assert ops.planes_of(xp) == ops.planes_mode() != 0
            y = conv(xp, doc, d)
            torch.cuda.synchronize()
            assert not ops.sync_error(dev()), 'a flag wait of the persistent launch gave up'
            e = _rel(y, K['ref'])
            print('planes GraphConv', kind, cin, cout, 'persistent' if persistent else 'tile per block', e)
            assert e <= 2e-5, (persistent, e)
    finally:
        ops.PLANES_MIN_TILES = saved
        _lib.call('ofx_set_gconv_persistent', 1)
    # backward against the oracle's autograd
    dx, dW = ops.graphconv_backward(xg, dyg, doc, d, Wg, nt)
    dx2, dW2 = ops.graphconv_backward(xg, dyg, doc, d, Wg, nt)
    assert torch.equal(dW, dW2), 'dW is not deterministic'
    assert torch.equal(dx, dx2), 'dx is not deterministic'
    o_doc = G.tree(kind)[1]
    floor = errors(_gconv_dx_ref(o_doc, d, K['dy'], K['W'], cin, nt, torch.float32), K['dx'])
    e, ew = errors(dx.cpu(), K['dx']), errors(dW, K['dW'])
    print('graphconv_backward', kind, cin, cout, 'dx', e, 'fp32 floor', floor, 'dW', ew)
    _within(e, floor, ('dx', kind, cin, cout))
    assert ew['rel_to_max'] <= 5e-5, ('dW', kind, cin, cout, ew)


def test_group_norm_backward_real_widths():
    """ofx_gn_backward at C = 256 / 512 / 768, 32 groups, ragged B = 8 (one element empty below the full layer)."""
    import torch.nn.functional as F
    import test_gpu_parity as P
    from octfusion_amd import ops
    from oracle import dual_octree as OD, modules as OM, sampler as OS
    split = C.random_split_small(8, 3, 58, p=0.4)
    split[2] = -1.0
    oc, doc = P.small(split)
    o_doc = OD.OracleDualOctree(OS.split2octree_small(split, 5, 3))
    o_doc.post_processing_for_docnn()
    d = 5
    N = doc.csr(d)[2]
    n = 0
    for Cc, act in [(256, 'silu'), (512, None), (768, 'silu')]:
        x = C.rand_input('gnx%d' % Cc, N, Cc) * 1.5 + 0.3
        dy = C.rand_input('gndy%d' % Cc, N, Cc)
        w = C.rand_input('gnw%d' % Cc, 1, Cc) * 0.5 + 1.0
        b = C.rand_input('gnb%d' % Cc, 1, Cc) * 0.2

        def ref(dtype):
            with torch.enable_grad():
                xs, ws_, bs = (t.to(dtype).requires_grad_(True) for t in (x, w, b))
                with OM.working_float(dtype):
                    y = OM.dual_octree_group_norm(xs, o_doc, d, ws_, bs, 32)
                if act == 'silu':
                    y = F.silu(y)
                (y * dy.to(dtype)).sum().backward()
            return xs.grad, ws_.grad.reshape(-1), bs.grad.reshape(-1)
        dx64, dg64, db64 = ref(torch.float64)
        dx32 = ref(torch.float32)[0]
        dx, dg, db = ops.group_norm_backward(x.to(dev()), dy.to(dev()), doc.batch_id32(d), doc.count(d), doc.batch_size,
                                             w.to(dev()), b.to(dev()), 32, act=act)
        floor, e = errors(dx32, dx64), errors(dx, dx64)
        report(dict(test='backward_fullwidth_group_norm', C=Cc, act=act, rows=N, dx=e, dx_reference_fp32_noise=floor,
                    dgamma=errors(dg, dg64), dbeta=errors(db, db64)))
        _within(e, floor, ('gn dx', Cc))
        assert _rel(dg, dg64) <= 2e-5 and _rel(db, db64) <= 2e-5
        n += 1
    assert n == 3


def test_attention_backward_real_sizes():
    """ofx_attention_bwd at the lr net's own attention sizes (snet: 8^3 tokens x 128 channels, 4^3 x 256; 4 heads)."""
    from octfusion_amd import ops
    n = 0
    for B, T, heads, ch in [(4, 512, 4, 32), (4, 64, 4, 64)]:
        Cc = heads * ch
        qkv = C.rand_input('attw%d_%d' % (T, ch), B * T, 3 * Cc)
        dout = C.rand_input('attwd%d_%d' % (T, ch), B * T, Cc)

        def ref(dtype):
            with torch.enable_grad():
                x = qkv.to(dtype).requires_grad_(True)
                t = x.view(B, T, heads, 3, ch).permute(0, 2, 3, 4, 1)
                q, k, v = t[:, :, 0], t[:, :, 1], t[:, :, 2]
                scale = 1 / math.sqrt(math.sqrt(ch))
                w = torch.softmax(torch.einsum('bhct,bhcs->bhts', q * scale, k * scale), dim=-1)
                o = torch.einsum('bhts,bhcs->bhct', w, v)
                (o.permute(0, 3, 1, 2).reshape(B * T, Cc) * dout.to(dtype)).sum().backward()
            return x.grad
        r64, r32 = ref(torch.float64), ref(torch.float32)
        got = ops.attention_backward(qkv.to(dev()), dout.to(dev()), B, T, heads)
        assert torch.equal(got, ops.attention_backward(qkv.to(dev()), dout.to(dev()), B, T, heads))
        floor, e = errors(r32, r64), errors(got, r64)
        report(dict(test='backward_fullwidth_attention', B=B, T=T, heads=heads, ch=ch, dqkv=e, reference_fp32_noise=floor))
        _within(e, floor, ('attention', T, ch))
        n += 1
    assert n == 2
