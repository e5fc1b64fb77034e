"""GroupNorm apply timings (GPU box): fp32 out / planes out / planes + folded aux rows, and the stand-alone pre-pass."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from octfusion_amd import _lib, ops, synthetic, modules as M
from octfusion_amd.dual_octree import DualOctree
from octfusion_amd.octree import split2octree_small
dev = torch.device('cuda:0')
torch.set_grad_enabled(False)
doc = DualOctree(split2octree_small(synthetic.shell6_split(8).to(dev), 6, 4))
def timeit(fn, n=30):
    for _ in range(3): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n
for d, C in [(6, 128), (6, 256), (6, 384), (5, 256), (5, 512), (4, 512)]:
    N = doc.csr(d)[2]
    gn = M.DualOctreeGroupNorm(C).to(dev)
    x = torch.randn(N, C, device=dev)
    bid, cnt = doc.batch_id32(d), doc.count(d)
    seg_ptr, col, _, _ = doc.csr(d)
    _, multi_seg, V = doc.ext(d)
    stats = torch.zeros(8 * C * 2, dtype=torch.float64, device=dev)
    _lib.call('ofx_gn_stats', x.data_ptr(), C, N, C, bid.data_ptr(), 8, stats.data_ptr(), torch.cuda.current_stream().cuda_stream)
    f = lambda **kw: ops.group_norm(x, bid, cnt, 8, gn.weights, gn.bias, gn.group, act='silu', stats=stats, **kw)
    t0 = timeit(lambda: f())
    t2 = timeit(lambda: f(planes=2))
    t2a = timeit(lambda: f(planes=2, aux_graph=ops.AuxGraph(seg_ptr, col, multi_seg, V)))
    plan = doc.aux_plan(d)
    t2p = timeit(lambda: f(planes=2, aux_graph=ops.AuxGraph(seg_ptr, col, multi_seg, V, block_plan=plan)))
    ya = f(planes=2, aux_graph=ops.AuxGraph(seg_ptr, col, multi_seg, V))
    yb = f(planes=2, aux_graph=ops.AuxGraph(seg_ptr, col, multi_seg, V, block_plan=plan))
    def aux_vals(y):
        a_ = getattr(y, ops.AUX_ATTR).view(torch.float32).view(V + 1, -1)[:, :C]
        setattr(a_, ops.PLANES_ATTR, 2)
        return ops.planes_merge(a_, 2)
    diff = float((aux_vals(ya) - aux_vals(yb)).abs().max())
    print('   aux rows by owner block (plan): %.1f us vs separate aux blocks %.1f us; leftover rows %d of %d; main rows equal %s, '
          'aux rows max |diff| %.2e' % (t2p, t2a, plan[1], V + 1, torch.equal(ya, yb), diff))
    # A/B: the separate ofx_gn_finalize launch (round 2) vs mean / rstd derived inside the apply launch (round 3)
    ops.GN_FINALIZE_LAUNCH = True
    t2a_sep = timeit(lambda: f(planes=2, aux_graph=ops.AuxGraph(seg_ptr, col, multi_seg, V)))
    t0_sep = timeit(lambda: f())
    ops.GN_FINALIZE_LAUNCH = False
    print('   finalize: fused %.1f / %.1f us (fp32 / planes+aux), separate launch %.1f / %.1f us' % (t0, t2a, t0_sep, t2a_sep))
    y = f(planes=2, aux_graph=ops.AuxGraph(seg_ptr, col, multi_seg, V))
    aux_fold = getattr(y, ops.AUX_ATTR).clone()
    # stand-alone pre-pass on the planes for comparison (timed through a conv-less call of the kernel is not exposed;
    # the aux rows of both paths must agree)
    yp = f(planes=2)
    ld = yp.stride(0) * 4
    aux2 = torch.empty((V + 1) * ld, dtype=torch.uint8, device=dev)
    print('d%d C=%d N=%d V=%d: fp32 %.1f us  planes %.1f us  planes+aux %.1f us  (bytes r+w %.0f MB -> %.2f TB/s fp32)' % (
        d, C, N, V, t0, t2, t2a, 8e-6 * N * C, 8e-6 * N * C / t0))
