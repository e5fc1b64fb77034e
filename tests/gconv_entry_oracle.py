"""float64 restatement of the fp32 gather-convolutions of csrc/ofx_gemm.hip (ofx_graphconv_fwd, ofx_graphconv_bwd_data,
ofx_gridconv_fwd, ofx_gridconv_bwd_data, ofx_gather_mean), written from the formulas of include/ofx.h ("GraphConv",
"Backward of GraphConv", "Backward of the 27-tap grid convolution", "Extended table"), with a derived elementwise bound per
precision, a bound for the fused statistics, a host emulation in fp32 that shows the bounds admit an honest
implementation (and planted errors that show they reject a dishonest one), a mirror of the entry points' choice between
the branch-free ("fast") path and the col path, and the shape tables the CPU and GPU tests share.  Nothing here imports
octfusion_amd.

Everything is stated in the PACKED k order of ofx_pack_weights / ofx_pack_conv3d: a col_data row is
[dir 0: cin | ... | dir 6: cin | zeros to pad32(7 cin) | dir * nt + t type fractions | zeros to pad32(7 nt)] (27 taps for
a grid) and the weight is `kernel_order(W)`, so a row of col_data times a column of the packed weight is the chain of
Kp terms the kernels add up.

Bounds (U = 2^-24; none of the constants is taken from a GPU result).
  contraction: gemm_oracle.bound for the precision's kind ('exact' under ofx_set_precision(1), 'fp16x3' under 3,
      'bf16x3' under 0) with chain = the k terms of one split-K slice of Kp and nsplit from the launcher's plan
      (gemm_oracle.plan on the fast path, per row chunk on the col path; no split with fused statistics).  emb is one more
      fp32 add after the bias fma and the residual add: chain + 1.
  aux / col rows of the forward: a segment of L > 1 sources is added serially in fp32 (L - 1 roundings) and scaled by the
      rounded 1 / L (two more; the col path divides, one more): within (L + 1) U mean|x| / (1 - (L + 1) U) of the mean.
      It enters the output times |W| of the slot's cin rows, for the slots with L > 1 only.
  aux / col rows of the backward: a weighted sum of L terms, each product rounded and added (or one fma): within
      2 L U sum|w x| / (1 - 2 L U), for every slot that is not a single edge of weight exactly 1.
  ofx_gather_mean: the same (L + 1) U mean|x| for L > 1; L <= 1 is a copy or a zero: exact.
  fused statistics: compared with float64 sums of the STORED output (stats_bound).  Depths read from the epilogues of
      csrc/ofx_gemm_common.h and the reducer of csrc/ofx_gemm.hip:
        float4 epilogue (epilogue_store_v4): a lane adds its 4 MI <= 8 rows serially in fp32, three butterfly steps add the
          8 lanes that share a column: depth 11 for a wave's 64 rows, with wave partials (stats_reduce_kernel adds them in
          fp64) and with atomics (fp64) alike; a wave that holds several batch elements keeps per-lane runs (<= 8).
        scalar epilogue (epilogue_store_scalar; always atomics): a lane owns a column and adds its 16 MI <= 32 rows
          serially, one fp64 atomic pair per run: depth 32.
      So STATS_DEPTH = partials 11, atomic 32 (the scalar epilogue; the float4 atomics stay within 11 and are held to 11).
      A sum of depth D is within D U sum|y| / (1 - D U); each square is rounded once more: (D + 1) U sum y^2; the fp64
      additions add 2^-41 of the same magnitudes.
"""
from types import SimpleNamespace

import numpy as np
import torch

import gemm_oracle as GM
import graph_oracle as GR
import gridtab_oracle as GT
from gconv_planes_oracle import labels
from gemm_oracle import U, assert_close, cdiv, check_window, pad32      # noqa: F401  (re-exported to the tests)

PRECISIONS = GM.PRECISIONS                      # ofx_set_precision: 1 exact fp32, 0 bf16x3, 3 fp16x3
PREC_NAME = {1: 'fp32', 0: 'bf16x3', 3: 'fp16x3'}
SIZES = (0, 1, 2, 8, 9, 3)
STATS_DEPTH = {'partials': 11, 'atomic_float4': 11, 'atomic': 32}


def kind(prec):
    return GM.kind_of(GM.flavour(prec, 4, 4, 0, gather=True))


def ntc(nt):
    """node-type columns that enter the contraction (ofx.h: type_frac may be NULL for nt <= 1)"""
    return nt if nt > 1 else 0


def nt_pad(nt):
    return pad32(7 * ntc(nt))


def packed_k(cin, nt, ndir=7):
    """ofx_graphconv_packed_k / ofx_conv3d_packed_k"""
    return pad32(ndir * cin) + nt_pad(nt)


def kernel_order(W, cin, nt, ndir=7):
    """fp32 [Kp, cout]: the reference rows dir * (cin + ntc) + c in the pack's k order"""
    t = ntc(nt)
    W3 = W.view(ndir, cin + t, -1)
    out = torch.zeros(packed_k(cin, nt, ndir), W.shape[1], dtype=W.dtype)
    out[:ndir * cin] = W3[:, :cin].reshape(ndir * cin, W.shape[1])
    kf = pad32(ndir * cin)
    out[kf:kf + ndir * t] = W3[:, cin:].reshape(ndir * t, W.shape[1])
    return out


# ------------------------------------------------------------------------------------------------ path predictor
def fast_path(cin, ldx, x_off=0, ext=True, aux=True, aux_off=0):
    """gather_common + the entries: the branch-free path needs cin % 32 == 0, ldx % 4 == 0, a 16-B aligned x, the extended
    table and a 16-B aligned aux (grid: zero_row); anything else is the col path.  Offsets in bytes."""
    return cin % 32 == 0 and ldx % 4 == 0 and x_off % 16 == 0 and bool(ext) and bool(aux) and aux_off % 16 == 0


def col_chunk(Kp, ws_bytes):
    """(rows per chunk, bytes of the tail) of launch_gather_via_col: the tail is ws_bytes / 8 (at most 16 MB, a multiple of
    16), the rest holds whole 128-row groups of Kp floats; fewer than 128 rows: OFX_EINVAL (chunk 0)."""
    tail = min(ws_bytes // 8, 16 << 20) & ~15
    chunk = (ws_bytes - tail) // (4 * Kp) // 128 * 128
    return (chunk if chunk >= 128 else 0), tail


def ws_for_chunk(Kp, rows):
    """smallest ws_bytes (a multiple of 128) whose col chunk is exactly `rows` (a multiple of 128)"""
    b = 4 * Kp * rows
    while col_chunk(Kp, b)[0] < rows:
        b += 128
    assert col_chunk(Kp, b)[0] == rows
    return b


def launch_plan(fast, n, cout, Kp, ws_bytes, stats, ws=True):
    """[(r0, rows, gemm_oracle.Plan)]: the dense / gather launches of one call.  Fused statistics take the workspace for
    their partials: a single pass."""
    if fast:
        return [(0, n, GM.plan(n, cout, Kp, ws_bytes, ws and not stats))]
    chunk, tail = col_chunk(Kp, ws_bytes)
    assert chunk, 'the col path needs room for 128 col rows'
    return [(r0, min(chunk, n - r0), GM.plan(min(chunk, n - r0), cout, Kp, tail, not stats)) for r0 in range(0, n, chunk)]


def stats_route(fast, n, cout, Kp, ws_bytes, vec4, ws_off=0):
    """'partials' (wave partials in the workspace, reduced in fp64) or 'atomic' / 'atomic_float4': launch_gemm keeps the
    partials only with the float4 epilogue, a 16-B aligned buffer and room for ceil(rows / wave rows) * cout * 8 bytes."""
    if not vec4:
        return 'atomic'
    wr = 32 if cout <= 32 else 64
    if fast:
        room, rows = ws_bytes, n
    else:
        chunk, room = col_chunk(Kp, ws_bytes)
        rows = min(chunk, n)
    return 'partials' if (ws_off % 16 == 0 and room > 0 and cdiv(rows, wr) * cout * 8 <= room) else 'atomic_float4'


# ------------------------------------------------------------------------------------------------ GraphConv forward
def make_case(n, cin, nt, cout, seed, sizes=SIZES, cuts=None, csr=None, node_type=None):
    """Operands of one GraphConv launch on the host: graph_oracle.hand_csr (segment r * 7 + dir), the tables built from
    it, x / W / bias / emb / res from gemm_oracle.operand / weight, the type fractions of a random node type rounded to
    fp32 (they are an fp32 operand of the entry: what the kernel reads is what the reference contracts).  csr / node_type:
    a given graph instead of the hand-made one."""
    g = torch.Generator().manual_seed(seed)
    t = ntc(nt)
    K = 7 * (cin + t)
    seg_ptr, col = csr if csr is not None else GR.hand_csr(seed, n, sizes=sizes)
    ext, multi = GR.primary_ext(seg_ptr, col, n)
    c = SimpleNamespace(n=n, cin=cin, nt=nt, ntc=t, nt_pad=nt_pad(nt), cout=cout, K=K, Kp=packed_k(cin, nt), seg_ptr=seg_ptr,
                        col=col, nbr=torch.from_numpy(GR.primary(seg_ptr, col)).view(n, 7),
                        ext=torch.from_numpy(ext).view(n, 7), multi=torch.from_numpy(multi),
                        L=torch.from_numpy(np.diff(seg_ptr)).view(n, 7))
    c.x = GM.operand((n, cin), seed + 1)
    c.W = GM.weight(K, cout, seed + 2)
    c.Wk = kernel_order(c.W, cin, nt)
    c.tf = torch.zeros(n, c.nt_pad)
    if t:
        if node_type is None:
            node_type = torch.randint(0, t, (n,), generator=g).numpy().astype(np.uint8)
        c.node_type = node_type
        c.tf[:, :7 * t] = torch.from_numpy(GR.type_frac(seg_ptr, col, node_type, t)[0]).reshape(n, 7 * t).float()
    cuts = cuts or [0, n // 3, n - n // 4, n]
    c.B = len(cuts) - 1
    c.bid = labels(n, cuts)
    c.bias = GM.operand((cout,), seed + 3)
    c.emb = GM.operand((c.B, cout), seed + 4)
    c.res = GM.operand((n, cout), seed + 5)
    return c


def seg_means(x, seg_ptr, col, w=None):
    """float64 (value [nseg, C], magnitude [nseg, C]): the mean over every segment of x[col] (zero for an empty one), or
    with weights w the weighted SUM; magnitude = the same of |w x|."""
    nseg = len(seg_ptr) - 1
    Ls = np.diff(seg_ptr)
    seg_of = torch.from_numpy(np.repeat(np.arange(nseg), Ls))
    src = x.double()[torch.from_numpy(np.asarray(col, dtype=np.int64))]
    if w is not None:
        src = src * torch.from_numpy(np.asarray(w, dtype=np.float32)).double()[:, None]
    val = torch.zeros(nseg, x.shape[1], dtype=torch.float64).index_add_(0, seg_of, src)
    mag = torch.zeros(nseg, x.shape[1], dtype=torch.float64).index_add_(0, seg_of, src.abs())
    if w is None:
        d = torch.from_numpy(np.maximum(Ls, 1)).double()[:, None]
        val, mag = val / d, mag / d
    return val, mag


def mean_err(L, mag):
    """[nseg, C]: (L + 1) U mean|x| / (1 - (L + 1) U) for L > 1, zero otherwise"""
    d = torch.as_tensor(L, dtype=torch.float64).reshape(-1, 1) + 1
    return torch.where(d > 2, d * U * mag / (1 - d * U), torch.zeros_like(mag))


def wsum_err(simple, L, mag):
    """[nseg, C]: 2 L U sum|w x| / (1 - 2 L U) for the segments that are not one edge of weight 1"""
    d = 2 * torch.as_tensor(L, dtype=torch.float64).reshape(-1, 1)
    e = d * U * mag / (1 - d * U)
    return torch.where(torch.as_tensor(simple).reshape(-1, 1), torch.zeros_like(e), e)


def col_data(c):
    """float64 ([n, Kp] col_data in packed k order, [n, Kp] the largest error of an honest fp32 col / aux row)"""
    mean, mag = seg_means(c.x, c.seg_ptr, c.col)
    A = torch.zeros(c.n, c.Kp, dtype=torch.float64)
    E = torch.zeros(c.n, c.Kp, dtype=torch.float64)
    A[:, :7 * c.cin] = mean.view(c.n, 7 * c.cin)
    E[:, :7 * c.cin] = mean_err(c.L.reshape(-1), mag).view(c.n, 7 * c.cin)
    kf = pad32(7 * c.cin)
    A[:, kf:] = c.tf.double()
    return A, E


def _finish(r, A, E, Wk, emb=None, bid=None):
    if emb is not None:
        e = emb.double()[bid.long()]
        r['ref'] = r['ref'] + e
        r['S'] = r['S'] + e.abs()
    r['A'] = A
    r['aux_term'] = E @ Wk.double().abs()
    return r


def reference(c, bias=True, emb=True, res=True):
    """out[r] = col_data[r] @ W + bias + emb[batch_id[r]] + res[r] in float64: the dict of gemm_oracle.gemm(full=True) plus
    A (col_data) and aux_term [n, cout] = sum_k (error of col_data[r, k]) |W[k, n]|."""
    A, E = col_data(c)
    r = GM.gemm(A, c.Wk, c.bias if bias else None, c.res if res else None, full=True)
    return _finish(r, A, E, c.Wk, c.emb if emb else None, c.bid)


def bound(prec, r, plans):
    """float64 [n, cout]: the largest admissible |got - ref| (module docstring); plans = launch_plan(...)"""
    b = torch.zeros_like(r['ref'])
    k = kind(prec)
    Kp = r['A'].shape[1]
    for r0, rows, p in plans:
        sl = slice(r0, r0 + rows)
        sub = dict(S=r['S'][sl], ref=r['ref'][sl], asum=r['asum'][sl], wsum=r['wsum'], wmax=r['wmax'])
        b[sl] = GM.bound(k, sub, GM.chain_len(Kp, p) + 1, p.nsplit)
    return b + r['aux_term'] * (1.0 + 2.0 ** -10)


# ------------------------------------------------------------------------------------------------ GraphConv backward
def make_bwd_case(n, cout, cin, seed, sizes=SIZES):
    """dx [n, cin] from dy [n, cout] over a weighted reverse CSR: hand_csr segments (c, dir) listing rows, hand_weights
    on its edges, so that multi-row segments carry weights other than 1 and single-row ones do too."""
    rev_ptr, rev_row = GR.hand_csr(seed, n, sizes=sizes)
    w = GR.hand_weights(seed, len(rev_row))
    ext, multi = GR.primary_ext_w(rev_ptr, rev_row, w, n)
    Ls = np.diff(rev_ptr)
    simple = np.array([GR._simple_w(rev_ptr, w, s) or Ls[s] == 0 for s in range(len(Ls))])
    c = SimpleNamespace(n=n, cin=cin, cout=cout, Kp=pad32(7 * cout), rev_ptr=rev_ptr, rev_row=rev_row, w=w,
                        nbr=torch.from_numpy(GR.primary_w(rev_ptr, rev_row, w)).view(n, 7), ext=torch.from_numpy(ext).view(n, 7),
                        multi=torch.from_numpy(multi), L=torch.from_numpy(Ls), simple=torch.from_numpy(simple))
    c.dy = GM.operand((n, cout), seed + 1)
    c.W = GM.weight(7 * cin, cout, seed + 2)                        # the forward weight, nt = 0
    c.WT = c.W.view(7, cin, cout).permute(0, 2, 1).reshape(7 * cout, cin).contiguous()
    c.Wk = kernel_order(c.WT, cout, 0)
    return c


def reference_bwd(c, weighted=True):
    """dx[c, :] = sum_dir (sum over reverse segment (c, dir) of rev_w dy[rev_row, :]) @ W_dir^T in float64"""
    w = c.w if weighted else np.ones_like(c.w)
    val, mag = seg_means(c.dy, c.rev_ptr, c.rev_row, w)
    A = torch.zeros(c.n, c.Kp, dtype=torch.float64)
    E = torch.zeros(c.n, c.Kp, dtype=torch.float64)
    A[:, :7 * c.cout] = val.view(c.n, -1)
    E[:, :7 * c.cout] = wsum_err(c.simple, c.L, mag).view(c.n, -1)
    return _finish(GM.gemm(A, c.Wk, full=True), A, E, c.Wk)


# ------------------------------------------------------------------------------------------------ grid convolution
def make_grid_case(mode, depth_out, B, cin, cout, seed):
    """27-tap convolution over gridtab_oracle.table (mode 0 same depth, 1 stride 2, 2 nearest-upsample + conv)"""
    n_in = GT.n_in(mode, depth_out, B)
    tab = GT.table(mode, depth_out, B, n_in)                        # padded with n_in: the zero row
    n_out = tab.shape[0]
    c = SimpleNamespace(mode=mode, n_in=n_in, n_out=n_out, n=n_out, cin=cin, cout=cout, B=B, Kp=pad32(27 * cin), tab=tab,
                        tab_m1=torch.where(tab == n_in, torch.full_like(tab, -1), tab))
    c.x = GM.operand((n_in, cin), seed + 1)
    c.weight = GM.weight(27 * cin, cout, seed + 2).view(27, cin, cout).permute(2, 1, 0).reshape(cout, cin, 3, 3, 3).contiguous()
    c.Wk = kernel_order(c.weight.reshape(cout, cin, 27).permute(2, 1, 0).reshape(27 * cin, cout).contiguous(), cin, 0, 27)
    c.bid = labels(n_out, [b * (n_out // B) for b in range(B + 1)])
    c.bias = GM.operand((cout,), seed + 3)
    c.emb = GM.operand((B, cout), seed + 4)
    c.res = GM.operand((n_out, cout), seed + 5)
    # backward: dy [n_out, cout] -> dx [n_in, cin] over the reverse table, unit weights
    c.dy = GM.operand((n_out, cout), seed + 6)
    _, rev_ptr, rev_row = GT.reverse(tab, n_in)
    c.rev_ptr, c.rev_row = np.asarray(rev_ptr, dtype=np.int64), np.asarray(rev_row, dtype=np.int64)
    c.w = np.ones(len(c.rev_row), dtype=np.float32)
    c.KpT = pad32(27 * cout)
    WT = c.weight.reshape(cout, cin, 27).permute(2, 0, 1).reshape(27 * cout, cin).contiguous()      # [tap * cout + o, c]
    c.weightT = c.weight.transpose(0, 1).contiguous()               # what ofx_pack_conv3d packs for the backward
    c.WkT = kernel_order(WT, cout, 0, 27)
    ext, multi = GR.primary_ext_w(c.rev_ptr, c.rev_row, c.w, n_out)
    c.rnbr = torch.from_numpy(GR.primary_w(c.rev_ptr, c.rev_row, c.w)).view(n_in, 27)
    c.rext, c.rmulti = torch.from_numpy(ext).view(n_in, 27), torch.from_numpy(multi)
    c.rL = torch.from_numpy(np.diff(c.rev_ptr))
    return c


def reference_grid(c, bias=True, emb=True, res=True, pad_row0=False):
    """out[r] = sum_tap x[nbr27[r, tap]] @ W_tap + bias + emb[bid[r]] + res[r]; a padded tap contributes nothing"""
    tab = c.tab
    A = torch.zeros(c.n_out, c.Kp, dtype=torch.float64)
    A[:, :27 * c.cin] = GM.gather_rows(c.x, tab)
    r = GM.gemm(A, c.Wk, c.bias if bias else None, c.res if res else None, full=True)
    return _finish(r, A, torch.zeros_like(A), c.Wk, c.emb if emb else None, c.bid)


def reference_grid_bwd(c):
    """dx[s] = sum over (r, tap) with nbr27[r, tap] == s of dy[r] @ W_tap^T"""
    val, mag = seg_means(c.dy, c.rev_ptr, c.rev_row, c.w)
    A = torch.zeros(c.n_in, c.KpT, dtype=torch.float64)
    E = torch.zeros(c.n_in, c.KpT, dtype=torch.float64)
    A[:, :27 * c.cout] = val.view(c.n_in, -1)
    E[:, :27 * c.cout] = wsum_err(c.rL <= 1, c.rL, mag).view(c.n_in, -1)
    return _finish(GM.gemm(A, c.WkT, full=True), A, E, c.WkT)


# ------------------------------------------------------------------------------------------------ gather mean
def gather_mean(x, seg_ptr, col):
    """(ref float64 [nseg, C], bound): ofx_gather_mean"""
    val, mag = seg_means(x, seg_ptr, col)
    return val, mean_err(np.diff(seg_ptr), mag)


# ------------------------------------------------------------------------------------------------ statistics
def stats_sums(y, bid, B):
    yd = y.detach().cpu().double()
    s = torch.zeros(B, yd.shape[1], 2, dtype=torch.float64)
    s[:, :, 0].index_add_(0, bid.long(), yd)
    s[:, :, 1].index_add_(0, bid.long(), yd * yd)
    mag = torch.zeros(B, yd.shape[1], dtype=torch.float64).index_add_(0, bid.long(), yd.abs())
    return s, mag


def stats_bound(y, bid, B, route):
    """(bS, bQ) float64 [B, cout]: admissible |stats - float64 sums of the stored y, y^2| (module docstring)"""
    D = STATS_DEPTH[route]
    s, mag = stats_sums(y, bid, B)
    return ((D * U / (1 - D * U) + 2.0 ** -41) * mag, ((D + 1) * U / (1 - (D + 1) * U) + 2.0 ** -41) * s[:, :, 1])


def emulate_stats(y, bid, B, route, mut=None):
    """float64 [B, cout, 2]: the fused statistics as the epilogues add them, in fp32 per 64-row wave and batch element
    (float4: 8 lanes x 8 rows serially, then a three-step butterfly; scalar: two lanes x 32 rows serially), waves added in
    fp64.  mut 'skip_after_boundary': the first row of every batch element but the first is left out."""
    y = y.float()
    n, C = y.shape
    keep = torch.ones(n, dtype=torch.bool)
    if mut == 'skip_after_boundary':
        keep[1:] = bid[1:] == bid[:-1]
    npad = cdiv(n, 64) * 64
    out = torch.zeros(B, C, 2, dtype=torch.float64)
    for b in range(B):
        on = ((bid == b) & keep).float()[:, None]
        for j, v in enumerate((y * on, y * y * on)):
            v = torch.cat([v, torch.zeros(npad - n, C)])
            if route == 'atomic':
                v = v.view(-1, 2, 32, C)
                acc = torch.zeros(v.shape[0], 2, C)
                for i in range(32):
                    acc = acc + v[:, :, i]
                out[b, :, j] = acc.double().sum((0, 1))
            else:
                v = v.view(-1, 8, 8, C)                        # [wave, step, lane]
                acc = torch.zeros(v.shape[0], 8, C)
                for i in range(8):
                    acc = acc + v[:, i]
                acc = acc[:, 0::2] + acc[:, 1::2]
                acc = acc[:, 0::2] + acc[:, 1::2]
                acc = acc[:, 0] + acc[:, 1]
                out[b, :, j] = acc.double().sum(0)
    return out


# ------------------------------------------------------------------------------------------------ host emulation
MUTATIONS = ('drop_dir', 'swap_type_dirs', 'wrong_count', 'emb_next', 'bias_twice', 'res_pitch', 'chunk_bid')
BWD_MUTATIONS = ('unweighted',)
GRID_MUTATIONS = ('pad_row0',)
RES_GAP = 4                                        # the emulation's res sits at pitch cout + RES_GAP; the gap holds 0.5


def applies(mut, c):
    """the shapes a planted error can show on"""
    if mut == 'swap_type_dirs':
        return c.ntc > 0
    if mut == 'wrong_count':
        return bool((c.L == 1).any())
    if mut == 'emb_next':
        return c.B > 1
    if mut == 'res_pitch':
        return c.n > 1
    if mut == 'chunk_bid':
        return c.n > 128 and not torch.equal(c.bid[128:], c.bid[:c.n - 128])
    return True


def _serial_mean(x, seg_ptr, col, w=None, count_plus=0.0):
    """fp32 [nseg, C]: the sources of every segment added serially in fp32; then times the rounded 1 / L (L > 1), or --
    with weights -- every term rounded after the product (no scaling).  count_plus: a one-source segment is divided by
    1 + count_plus (the planted error)."""
    nseg = len(seg_ptr) - 1
    sp = np.asarray(seg_ptr, dtype=np.int64)
    Ln = np.diff(sp)
    Ls = torch.from_numpy(Ln)
    seg_of = np.repeat(np.arange(nseg), Ln)
    pos = np.arange(int(sp[-1])) - np.repeat(sp[:-1], Ln)
    src = torch.zeros(nseg, int(Ln.max()) if nseg else 0, dtype=torch.int64)
    ww = torch.zeros(src.shape)
    src[seg_of, pos] = torch.from_numpy(np.asarray(col, dtype=np.int64))
    ww[seg_of, pos] = 1.0 if w is None else torch.from_numpy(np.asarray(w, dtype=np.float32))
    acc = torch.zeros(nseg, x.shape[1])
    for p in range(src.shape[1]):
        acc = acc + x[src[:, p]] * ww[:, p:p + 1]
    if w is None:
        cnt = Ls.float().clamp(min=1.0)
        cnt = torch.where(Ls == 1, cnt + count_plus, cnt)
        acc = torch.where((cnt != 1.0)[:, None], acc * (torch.ones(nseg) / cnt)[:, None], acc)
    return acc


def _contract(prec, A, Wk, bias, plans):
    out = torch.zeros(A.shape[0], Wk.shape[1])
    for r0, rows, p in plans:
        out[r0:r0 + rows] = GM.emulate(kind(prec), A[r0:r0 + rows], Wk, bias, None, p)
    return out


def emulate(c, prec, plans, bias=True, emb=True, res=True, mut=None):
    """fp32 [n, cout]: ofx_graphconv_fwd on the host -- the means by _serial_mean, the contraction by gemm_oracle.emulate
    in the precision's kind per launch of `plans`, then emb and res added.  `mut`: one of MUTATIONS."""
    n, cin = c.n, c.cin
    A = torch.zeros(n, c.Kp)
    rows = _serial_mean(c.x, c.seg_ptr, c.col, count_plus=1.0 if mut == 'wrong_count' else 0.0).view(n, 7, cin)
    if mut == 'drop_dir':
        rows[:, 3] = 0.0
    A[:, :7 * cin] = rows.reshape(n, 7 * cin)
    kf = pad32(7 * cin)
    tf = c.tf[:, :7 * c.ntc].view(n, 7, c.ntc)
    if mut == 'swap_type_dirs':
        tf = tf[:, [1, 0, 2, 3, 4, 5, 6]]
    A[:, kf:kf + 7 * c.ntc] = tf.reshape(n, 7 * c.ntc)
    out = _contract(prec, A, c.Wk, c.bias if bias else None, plans)
    if bias and mut == 'bias_twice':
        out = out + c.bias
    if emb:
        bid = c.bid.long().clone()
        if mut == 'emb_next':
            bid = (bid + 1) % c.B
        if mut == 'chunk_bid':
            for r0 in range(128, n, 128):
                bid[r0:r0 + 128] = c.bid.long()[:min(128, n - r0)]
        out = out + c.emb[bid]
    if res:
        rr = c.res
        if mut == 'res_pitch':
            buf = torch.full((n, c.cout + RES_GAP), 0.5)
            buf[:, :c.cout] = c.res
            rr = buf.reshape(-1)[:n * c.cout].view(n, c.cout)
        out = out + rr
    return out


def emulate_bwd(c, prec, plans, mut=None):
    A = torch.zeros(c.n, c.Kp)
    w = np.ones_like(c.w) if mut == 'unweighted' else c.w
    A[:, :7 * c.cout] = _serial_mean(c.dy, c.rev_ptr, c.rev_row, w).view(c.n, -1)
    return _contract(prec, A, c.Wk, None, plans)


def emulate_grid(c, prec, plans, bias=True, emb=True, res=True, mut=None):
    tab = c.tab.long().clone()
    xz = torch.cat([c.x, torch.zeros(1, c.cin)])
    if mut == 'pad_row0':
        tab[tab == c.n_in] = 0
    A = torch.zeros(c.n_out, c.Kp)
    A[:, :27 * c.cin] = xz[tab].reshape(c.n_out, -1)
    out = _contract(prec, A, c.Wk, c.bias if bias else None, plans)
    if emb:
        out = out + c.emb[c.bid.long()]
    if res:
        out = out + c.res
    return out


def emulate_grid_bwd(c, prec, plans):
    A = torch.zeros(c.n_in, c.KpT)
    A[:, :27 * c.cout] = _serial_mean(c.dy, c.rev_ptr, c.rev_row, c.w).view(c.n_in, -1)
    return _contract(prec, A, c.WkT, None, plans)


# ------------------------------------------------------------------------------------------------ shared shape tables
NS = (1, 63, 129, 300)
# (name, n, cin, nt, cout): cin 32 / 64 fast, 3 / 24 col; nt 0 / 4 / 5 -> nt_pad 0 / 32 / 64; every column tile, cout % 4
FWD_SHAPES = [('n1', 1, 32, 0, 36), ('n63', 63, 64, 4, 3), ('n129', 129, 32, 5, 130), ('n300', 300, 64, 5, 64),
              ('n129b', 129, 64, 0, 130), ('n63b', 63, 32, 4, 64),
              ('col_n1', 1, 3, 4, 64), ('col_n63', 63, 24, 0, 130), ('col_n129', 129, 3, 5, 36), ('col_n300', 300, 24, 4, 3),
              ('col_n129b', 129, 24, 5, 64), ('col_n63b', 63, 3, 0, 3)]
TRIGGER_SHAPE = ('trig', 129, 64, 4, 36)
TRIGGERS = ('none', 'no_ext', 'aux_null', 'aux_off', 'x_off', 'ldx')
PITCH_SHAPE = ('pitch', 129, 32, 5, 36)
PITCHES = ('ldx', 'ldt', 'ldc', 'ldr', 'lde', 'stats_ld', 'all')
EPILOGUES = {'none': (False, False, False), 'bias': (True, False, False), 'emb': (False, True, False),
             'res': (False, False, True), 'all': (True, True, True)}
EPI_SHAPE = ('epi', 129, 32, 4, 36)
STATS_SHAPE_V4 = ('stats', 300, 64, 4, 36)
STATS_SHAPE_S = ('stats3', 300, 64, 4, 3)
# three batch elements and an empty one (label 2): a cut inside the first wave tile, inside the second 128-row chunk,
# and exactly on the chunk boundary 256
STATS_CUTS = [0, 40, 200, 200, 256, 300]
NOMULTI_SHAPE = ('nomulti', 129, 64, 4, 36)
NOMULTI_SIZES = (0, 1, 1)
BWD_SHAPES = [('b32', 129, 32, 36), ('b64', 300, 64, 24), ('b3', 63, 3, 32), ('b24', 129, 24, 5), ('b1', 1, 32, 64)]
GRID_TABLES = [(mode, d, B) for mode in (0, 1, 2) for d in (1, 2) for B in (1, 3)]
GRID_WIDTHS = ((32, 36), (3, 32), (16, 24))          # (cin, cout): forward fast / col / col, backward col / fast / col
GATHER_MEAN_SIZES = (0, 1, 2, 255, 256, 1000)
ALL_FWD = FWD_SHAPES + [TRIGGER_SHAPE, PITCH_SHAPE, EPI_SHAPE, STATS_SHAPE_V4, STATS_SHAPE_S, NOMULTI_SHAPE]

_CASES = {}


def case(shape, sizes=SIZES, cuts=None):
    """make_case of a table row, built once and left unchanged"""
    name, n, cin, nt, cout = shape
    key = (name, sizes, tuple(cuts) if cuts else None)
    if key not in _CASES:
        _CASES[key] = make_case(n, cin, nt, cout, 11 * n + cout + cin, sizes, cuts)
    return _CASES[key]


def bwd_case(shape):
    name, n, cout, cin = shape
    if ('bwd', name) not in _CASES:
        _CASES[('bwd', name)] = make_bwd_case(n, cout, cin, 13 * n + cout + cin)
    return _CASES[('bwd', name)]


def grid_case(mode, d, B, cin, cout):
    key = ('grid', mode, d, B, cin, cout)
    if key not in _CASES:
        _CASES[key] = make_grid_case(mode, d, B, cin, cout, 100 * mode + 10 * d + B + cin)
    return _CASES[key]


def vec4(cout, ldc, out_off=0, res=False, ldr=0, res_off=0, emb=False, lde=0, bias_off=0):
    """float4 epilogue of launch_gemm: gemm_oracle.vec4 and an emb pitch % 4 == 0"""
    return GM.vec4(cout, ldc, out_off, res, ldr, res_off, bias_off) and (not emb or lde % 4 == 0)


# ================================================================================================ narrow convolutions
# The two gather-shaped GraphConvs of csrc/ofx_narrow.hip, raw weights W [7 (cin + nt), cout] in the REFERENCE's row
# order dir * (cin + nt) + c (nt is taken as given: no nt > 1 rule here).
#
# ofx_graphconv_narrow_in / _tab (exact fp32): col_data[r, dir * (cin + nt) + c] = the segment mean, added serially in fp32
#     and scaled by __frcp_rn(L) (correctly rounded: one rounding, the product one more): (L + 1) U mean|x| for L > 1, exact
#     for L <= 1; a type fraction is an exact count times the rounded 1 / L: 2 U f (L > 1).  Then a chain of KP fmas
#     (KP = the kernel's padded K: 64 / 72 / 96) and the bias add: (KP + 1) U S.
# ofx_graphconv_narrow_out: per direction the sum of L rows of P, serially, divided by L: (L + 1) U mean|P| (L > 1); the seven
#     means and the type term meet by three butterfly additions: 3 U (sum_dir |mean| + |type term|).
# ofx_narrow_out_type_term: per direction an fma chain over nt types, then the same butterfly with the bias as the eighth
#     lane: held to (7 nt + 1) U (sum |f w| + |bias|).
# ofx_narrow_out_pack: a permutation with zero fill: bit-exact.
# fused statistics of narrow_in: a lane adds the 16 rows of its tile serially, one shuffle adds the other half of the tile,
#     one addition the second row tile of the 64-row group: depth 18; groups are added in fp64 (stats_reduce_kernel); a
#     group that holds two batch elements uses fp64 atomics per value.
STATS_DEPTH['narrow'] = 18
NARROW_KP = {False: lambda K: 64 if K <= 64 else 96, True: lambda K: 64 if K <= 64 else (72 if K <= 72 else 96)}
# (cin, nt): every instantiation of narrow_in_kernel<64 | 96, 4 | 8> and narrow_in2_kernel<64 | 72 | 96, 4 | 8>
NARROW_IN_WIDTHS = [(1, 0), (3, 0), (3, 5), (4, 5), (5, 0), (8, 0), (8, 1), (3, 7), (4, 6), (5, 5), (8, 2), (3, 8), (4, 8),
                    (5, 8), (8, 5)]
NARROW_IN_REFUSED = [(8, 6), (6, 8)]
NARROW_NS = (1, 63, 64, 65, 200)


def narrow_inst(cin, nt, tab):
    """(KP, CI) of the kernel instantiation"""
    return NARROW_KP[tab](7 * (cin + nt)), 4 if cin <= 4 else 8


def make_narrow_in(n, cin, nt, cout, seed, sizes=SIZES, cuts=None, one_type=None):
    """one_type = L: the segment of L sources is made of nodes of a single type (type 0)"""
    g = torch.Generator().manual_seed(seed)
    seg_ptr, col = GR.hand_csr(seed, n, sizes=sizes)
    col = col.copy()
    node_type = torch.randint(0, max(nt, 1), (n,), generator=g).numpy().astype(np.uint8)
    node_type[0] = 0
    if one_type is not None:
        s = int(np.nonzero(np.diff(seg_ptr) == one_type)[0][0])
        zeros = np.nonzero(node_type == 0)[0]
        col[seg_ptr[s]:seg_ptr[s + 1]] = zeros[np.arange(one_type) % len(zeros)]
    ext, multi = GR.primary_ext_fast(seg_ptr, col, n)
    K = 7 * (cin + nt)
    c = SimpleNamespace(n=n, cin=cin, nt=nt, cout=cout, K=K, seg_ptr=seg_ptr, col=col, node_type=node_type,
                        ext=torch.from_numpy(ext).view(n, 7), multi=torch.from_numpy(multi),
                        L=torch.from_numpy(np.diff(seg_ptr)).view(n, 7), one_type=one_type)
    c.x = GM.operand((n, cin), seed + 1)
    c.W = GM.weight(K, cout, seed + 2)
    c.bias = GM.operand((cout,), seed + 3)
    cuts = cuts or [0, n // 3, n - n // 4, n]
    c.B = len(cuts) - 1
    c.bid = labels(n, cuts)
    return c


def reference_narrow_in(c, bias=True):
    """float64: col_data @ W + bias, with E = the largest error of an honest fp32 col_data"""
    n, cin, nt = c.n, c.cin, c.nt
    mean, mag = seg_means(c.x, c.seg_ptr, c.col)
    A = torch.zeros(n, 7, cin + nt, dtype=torch.float64)
    E = torch.zeros(n, 7, cin + nt, dtype=torch.float64)
    A[:, :, :cin] = mean.view(n, 7, cin)
    E[:, :, :cin] = mean_err(c.L.reshape(-1), mag).view(n, 7, cin)
    if nt:
        f = torch.from_numpy(GR.type_frac_fast(c.seg_ptr, c.col, c.node_type, nt)[0]).view(n, 7, nt)
        A[:, :, cin:] = f
        E[:, :, cin:] = torch.where((c.L > 1)[:, :, None], 2 * U * f, torch.zeros_like(f))
    A, E = A.reshape(n, c.K), E.reshape(n, c.K)
    r = GM.gemm(A, c.W, c.bias if bias else None, full=True)
    return _finish(r, A, E, c.W)


def bound_narrow_in(r, KP):
    cc = KP + 1
    return (cc * U * r['S'] + r['aux_term']) * (1.0 + 2.0 ** -10) / (1.0 - cc * U)


def _byte_counts(cnt):
    """[nseg, 8] counts as the aux record of narrow_rec_aux_kernel holds them: two u32 words, one byte per type"""
    out = np.zeros_like(cnt)
    for h in (0, 4):
        word = np.zeros(cnt.shape[0], dtype=np.int64)
        for t in range(4):
            word = (word + (cnt[:, h + t] << (8 * t))) & 0xFFFFFFFF
        for t in range(4):
            out[:, h + t] = (word >> (8 * t)) & 255
    return out


def emulate_narrow_in(c, tab=False, bias=True, mut=None):
    """fp32 [n, cout]: the means by _serial_mean, the type fractions as exact count * rounded 1 / L -- with tab=True the
    counts of a multi-neighbour segment pass through one byte per type (the stated limit of ofx_graphconv_narrow_in_tab) --,
    then the fma chain.  mut: 'drop_dir', 'wrong_count', 'bias_twice'."""
    n, cin, nt = c.n, c.cin, c.nt
    A = torch.zeros(n, 7, cin + nt)
    A[:, :, :cin] = _serial_mean(c.x, c.seg_ptr, c.col, count_plus=1.0 if mut == 'wrong_count' else 0.0).view(n, 7, cin)
    if nt:
        cnt = GR.type_frac_fast(c.seg_ptr, c.col, c.node_type, nt)[1]
        full = np.zeros((cnt.shape[0], 8), dtype=np.int64)
        full[:, :nt] = cnt
        if tab:
            multi = np.diff(c.seg_ptr) > 1
            full[multi] = _byte_counts(full[multi])
        inv = torch.ones(n * 7) / c.L.reshape(-1).float().clamp(min=1.0)
        A[:, :, cin:] = (torch.from_numpy(full[:, :nt]).float() * inv[:, None]).view(n, 7, nt)
    if mut == 'drop_dir':
        A[:, 3] = 0.0
    out = GM.emulate('exact', A.reshape(n, c.K), c.W, c.bias if bias else None, None, GM.plan(n, c.cout, c.K, ws=False))
    return out + c.bias if (bias and mut == 'bias_twice') else out


# ------------------------------------------------------------------------------------------------ narrow output side
def pack_reference(W, C, nt, cout, pw):
    """Wd [C, pw]: Wd[c, dir * cout + o] = W[dir * (C + nt) + c, o], zero beyond 7 cout"""
    Wd = torch.zeros(C, pw)
    Wd[:, :7 * cout] = W.view(7, C + nt, cout)[:, :C].permute(1, 0, 2).reshape(C, 7 * cout)
    return Wd


def type_term(tf, nt, W, C, cout, bias):
    """(ref float64 [n, cout], bound): bias[o] + sum_{dir, t} tf[r, dir * nt + t] W[dir * (C + nt) + C + t, o]"""
    n = tf.shape[0]
    Wt = W.double().view(7, C + nt, cout)[:, C:].reshape(7 * nt, cout)
    f = tf.double()[:, :7 * nt]
    ref, S = f @ Wt, f.abs() @ Wt.abs()
    if bias is not None:
        ref, S = ref + bias.double(), S + bias.double().abs()
    d = 7 * nt + 1
    return ref.reshape(n, cout), d * U * S * (1.0 + 2.0 ** -10) / (1 - d * U)


def _butterfly8(v):
    """[n, 8, C] fp32 -> [n, C]: lanes added by xor 1, 2, 4"""
    v = v[:, 0::2] + v[:, 1::2]
    v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0] + v[:, 1]


def emulate_type_term(tf, nt, W, C, cout, bias):
    n = tf.shape[0]
    Wt = W.view(7, C + nt, cout)[:, C:]
    lanes = torch.zeros(n, 8, cout)
    for t in range(nt):
        lanes[:, :7] = GM._fma32(lanes[:, :7], tf[:, :7 * nt].reshape(n, 7, nt)[:, :, t:t + 1], Wt[None, :, t])
    if bias is not None:
        lanes[:, 7] = bias
    return _butterfly8(lanes)


def reference_narrow_out(P, cout, seg_ptr, col, tt):
    """(ref float64 [n, cout], bound): sum_dir mean_{e in seg(r, dir)} P[col[e], dir * cout + o] + tt[r, o]"""
    n = (len(seg_ptr) - 1) // 7
    mean, mag = seg_means(P[:, :7 * cout], seg_ptr, col)                      # [n * 7, 7 cout]
    pick = (torch.arange(n * 7) % 7)[:, None] * cout + torch.arange(cout)[None, :]
    mean, mag = mean.gather(1, pick).view(n, 7, cout), mag.gather(1, pick).view(n, 7, cout)
    err = mean_err(np.diff(seg_ptr), mag.view(n * 7, cout)).view(n, 7, cout).sum(1)
    ref, S = mean.sum(1), mag.sum(1)
    if tt is not None:
        ref, S = ref + tt.double(), S + tt.double().abs()
    return ref, (err + 3 * U * S) * (1.0 + 2.0 ** -10) / (1 - 3 * U), S


def emulate_narrow_out(P, cout, seg_ptr, col, tt, mut=None):
    n = (len(seg_ptr) - 1) // 7
    Ls = torch.from_numpy(np.diff(seg_ptr)).float().clamp(min=1.0)
    s = _serial_mean(P[:, :7 * cout], seg_ptr, col, w=np.ones(len(col), dtype=np.float32))      # plain serial sums
    pick = (torch.arange(n * 7) % 7)[:, None] * cout + torch.arange(cout)[None, :]
    if mut == 'swap_dirs':
        pick = ((torch.arange(n * 7) + 1) % 7)[:, None] * cout + torch.arange(cout)[None, :]
    lanes = torch.zeros(n, 8, cout)
    lanes[:, :7] = (s.gather(1, pick) / Ls[:, None]).view(n, 7, cout)
    if tt is not None:
        lanes[:, 7] = tt
    return _butterfly8(lanes)
