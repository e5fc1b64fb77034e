"""float64 restatement of the GraphConv on operand planes (ofx_graphconv_fwd_planes / _cus, ofx_pack_weights_planes,
ofx_planes_split and the aux rows of planes_multi_mean), written from the formulas of include/ofx.h ("GraphConv",
"GraphConv on operand planes", "Extended table", ofx_graph_type_frac, the range guard), with ONE derived elementwise bound
per contraction mode, a bound for the fused statistics, a host emulation that shows the bounds admit an honest
implementation (and planted errors that show they reject a dishonest one), the expected bytes of the weight pack, and
the shape tables the CPU and GPU tests share.  Nothing here imports octfusion_amd.

What the kernel reads is exactly decode(planes): the activations and the type fractions are encoded once on the host
(gn_oracle.encode) and the reference contracts the DECODED values, so a directly gathered row and a type row carry no
operand error of their own; only the weights (split at pack time) and the aux rows (an fp32 mean, split again) do.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

import gemm_oracle as GM
import gn_oracle as GN
import graph_oracle as GR
from gemm_oracle import U, assert_close, cdiv, weight_scale      # noqa: F401  (assert_close: re-exported to the tests)

LINE = 128                      # bytes of one k tile of one row
MODES = (3, 2, 1)               # fp16 pairs, bf16 pairs, single fp16
MODE_NAME = {3: 'fp16x3', 2: 'bf16x3', 1: 'fp16'}
TILES = (2, 4)                  # ofx_set_gconv2_tile: 128-row and 256-row blocks


def pairs(mode):
    return mode in (2, 3)


def chunk(mode):
    """channels per 128-B line"""
    return 32 if pairs(mode) else 64


def bpc(mode):
    """bytes per channel of a planes row"""
    return 4 if pairs(mode) else 2


def ntc(nt):
    """node-type columns that enter the contraction (ofx.h: type_frac may be NULL for nt <= 1)"""
    return nt if nt > 1 else 0


def type_tiles(nt, mode):
    return cdiv(7 * ntc(nt), chunk(mode))


def ktiles(cin, nt, mode):
    """ofx_planes_packed_ktiles by the header: 7 cin gathered channels, then the 7 nt type rows padded to a whole tile"""
    return 7 * (cin // chunk(mode)) + type_tiles(nt, mode)


def packed_bytes(cin, nt, cout, mode):
    """ofx_planes_packed_bytes: [k tile][cout][128 B] + the 128-B trailer [1 / s, s]"""
    return ktiles(cin, nt, mode) * cout * LINE + LINE


def ni_of(cout):
    return 1 if cout <= 64 else 2


def is_vec4(cout, ldc, out_off=0, res=True, ldr=0, res_off=0, emb=True, lde=0, bias=True, bias_off=0):
    """float4 epilogue (offsets in bytes against a 16-B aligned base)"""
    return (cout % 4 == 0 and ldc % 4 == 0 and out_off % 16 == 0 and (not res or (ldr % 4 == 0 and res_off % 16 == 0)) and
            (not emb or lde % 4 == 0) and (not bias or bias_off % 16 == 0))


# ------------------------------------------------------------------------------------------------ cases
# planted operands whose lo half is large in BOTH pair formats, so that a dropped cross term shows in one element:
#   activation 64.2185: fp16 hi 64.1875 lo 0.031 (4.8e-4 of it), bf16 hi 64 lo 0.2185
#   weight 40.108398: times the pack's scale 512 it is 20535.5 -> fp16 hi 20528 lo 7.5 (3.7e-4), bf16 hi 40 lo 0.1084
PROBE_A, PROBE_W, PROBE_C, PROBE_N = 64.2185, 40.108398, 5, 1


def labels(n, cuts):
    bid = torch.zeros(n, dtype=torch.int32)
    for b in range(len(cuts) - 1):
        bid[cuts[b]:cuts[b + 1]] = b
    return bid


def make_case(n, cin, nt, cout, mode, seed, sizes=(0, 1, 2, 8, 9, 3), cuts=None):
    """Operands of one launch, on the host.  The CSR is graph_oracle.hand_csr (segment r * 7 + dir; sizes drawn from the
    first three of `sizes`, each of `sizes` planted once); x = randn with every 7th element zero; W = randn / sqrt(K) with
    every 7th element zero; one probe pair (above) planted on a directly gathered row.  Batch labels: `cuts` or three
    nearly equal runs."""
    g = torch.Generator().manual_seed(seed)
    t = ntc(nt)
    K = 7 * (cin + t)
    seg_ptr, col = GR.hand_csr(seed, n, sizes=sizes)
    ext, multi = GR.primary_ext(seg_ptr, col, n)
    x = torch.randn(n, cin, generator=g)
    x.reshape(-1)[3::7] = 0.0
    W = torch.randn(K, cout, generator=g) / math.sqrt(K)
    W.reshape(-1)[2::7] = 0.0
    single = np.nonzero(np.diff(seg_ptr) == 1)[0]
    probe = None
    if len(single):
        s = int(single[len(single) // 2])
        x[int(col[seg_ptr[s]]), PROBE_C] = PROBE_A
        W[(s % 7) * (cin + t) + PROBE_C, min(PROBE_N, cout - 1)] = PROBE_W
        probe = (s // 7, min(PROBE_N, cout - 1))
    planes = GN.encode(x, mode)
    c = SimpleNamespace(n=n, cin=cin, nt=nt, ntc=t, cout=cout, mode=mode, K=K, seg_ptr=seg_ptr, col=col,
                        ext=torch.from_numpy(ext).view(n, 7), multi=torch.from_numpy(multi), probe=probe,
                        x=x, W=W, planes=planes, xd=GN.decode(planes, cin, mode), nkt=ktiles(cin, nt, mode))
    c.seg_len = torch.from_numpy(np.diff(seg_ptr)).view(n, 7)
    c.multi_mask = c.ext > n
    if t:
        node_type = torch.randint(0, t, (n,), generator=g).numpy().astype(np.uint8)
        frac = GR.type_frac(seg_ptr, col, node_type, t)[0]
        tf = torch.zeros(n, type_tiles(nt, mode) * chunk(mode))
        tf[:, :7 * t] = torch.from_numpy(frac).reshape(n, 7 * t).float()
        c.tplanes = GN.encode(tf, mode)
        c.tfd = GN.decode(c.tplanes, tf.shape[1], mode)[:, :7 * t]
    else:
        c.tplanes, c.tfd = None, torch.zeros(n, 0, dtype=torch.float64)
    cuts = cuts or [0, n // 3, n - n // 4, n]
    c.B = len(cuts) - 1
    c.bid = labels(n, cuts)
    c.bias = torch.randn(cout, generator=g)
    c.emb = torch.randn(c.B, cout, generator=g)
    c.res = torch.randn(n, cout, generator=g)
    return c


# ------------------------------------------------------------------------------------------------ aux rows
def _seg_sources(c):
    """(src [V, Lmax] source rows padded with row 0, L [V] lengths) of the multi-neighbour segments"""
    V = len(c.multi)
    L = torch.tensor([int(c.seg_ptr[s + 1] - c.seg_ptr[s]) for s in c.multi.tolist()], dtype=torch.int64)
    src = torch.zeros(V, int(L.max()) if V else 1, dtype=torch.int64)
    for v, s in enumerate(c.multi.tolist()):
        a, e = int(c.seg_ptr[s]), int(c.seg_ptr[s + 1])
        src[v, :e - a] = torch.from_numpy(c.col[a:e].astype(np.int64))
    return src, L


def aux(c):
    """(mean float64 [V + 1, cin], bytes uint8 [V + 1, cin * bpc]): ofx.h "Extended table" -- row 0 the zero row, row
    1 + v the mean of the decoded source rows of segment multi_seg[v]; the bytes an honest kernel stores for it."""
    src, L = _seg_sources(c)
    mean = torch.zeros(len(L) + 1, c.cin, dtype=torch.float64)
    if len(L):
        on = (torch.arange(src.shape[1])[None, :] < L[:, None]).double()
        mean[1:] = (c.xd[src] * on[:, :, None]).sum(1) / L[:, None].double()
    return mean, GN.encode(mean.float(), c.mode)


def split_err(mode, mag):
    """|v - stored(v)| for an fp32 v, |v| <= mag, written in the mode's format:
      fp16 pairs: hi within 2^-11 |v|, v - hi exact in fp32, lo rounds it to 11 bits or -- an fp16 denormal -- to a
                  multiple of 2^-24: 2^-22 |v| + 2^-25;
      bf16 pairs: 8 + 8 bits, fp32's exponent range: 2^-16 |v|;
      fp16:       2^-11 |v| + 2^-25."""
    if mode == 3:
        return 2.0 ** -22 * mag + 2.0 ** -25
    if mode == 2:
        return 2.0 ** -16 * mag
    return 2.0 ** -11 * mag + 2.0 ** -25


def aux_err(c):
    """[V + 1, cin]: the largest |stored aux value - float64 mean|.  The kernel adds the L decoded sources serially in fp32
    (L - 1 roundings), multiplies by the rounded 1 / L (two more): (L + 1) U mean|x| / (1 - (L + 1) U); the result is
    split into the mode's format (split_err of |mean| + that).  Row 0 is exact zeros."""
    src, L = _seg_sources(c)
    out = torch.zeros(len(L) + 1, c.cin, dtype=torch.float64)
    if len(L):
        on = (torch.arange(src.shape[1])[None, :] < L[:, None]).double()
        mabs = (c.xd[src].abs() * on[:, :, None]).sum(1) / L[:, None].double()
        d = (L[:, None].double() + 1)
        e = d * U * mabs / (1 - d * U)
        out[1:] = e + split_err(c.mode, mabs + e)
    return out


# ------------------------------------------------------------------------------------------------ reference
def col_data(c, mean=None):
    """float64 [n, 7 (cin + ntc)] in the REFERENCE's row order dir * (cin + ntc) + c (ofx.h "GraphConv": the 7 direction
    means, then -- per direction -- the type fractions)."""
    mean = aux(c)[0] if mean is None else mean
    rows = torch.cat([c.xd, mean])[c.ext.long()]                               # [n, 7, cin]
    return torch.cat([rows, c.tfd.view(c.n, 7, c.ntc)], 2).reshape(c.n, c.K)


def reference(c, bias=True, emb=True, res=True):
    """out[r] = col_data[r] @ W + bias + emb[batch_id[r]] + res[r] in float64.  A dict in the layout of
    gemm_oracle._contract: ref, S = sum_k |a_k| |w_k| + |bias| + |emb| + |res|, asum, wsum, wmax, written (all rows), plus
    what `bound` needs for the aux slots: aux_term [n, cout] = sum over the (row, dir) slots that gather an aux row of
    aux_err |w|, and A (col_data)."""
    A = col_data(c)
    r = GM.gemm(A, c.W, c.bias if bias else None, c.res if res else None, full=True)
    if emb:
        e = c.emb.double()[c.bid.long()]
        r['ref'] = r['ref'] + e
        r['S'] = r['S'] + e.abs()
    E = torch.cat([aux_err(c), torch.zeros(1, c.cin, dtype=torch.float64)])              # last row: not an aux slot
    idx = torch.where(c.multi_mask, c.ext.long() - c.n, torch.full_like(c.ext.long(), E.shape[0] - 1))
    Eslot = torch.cat([E[idx], torch.zeros(c.n, 7, c.ntc, dtype=torch.float64)], 2)     # [n, 7, cin + ntc]
    r['aux_slot_err'] = Eslot
    r['A'], r['Wabs'] = A, c.W.double().abs()
    return r


def bound(mode, r, chain, pieces, multi_mask):
    """Largest admissible |got - ref| per element, float64 [n, cout].  r = reference(...), chain = nkt * chunk (the k
    terms of one output element, padding included), pieces = the partial sums of one tile the persistent launch adds in k
    order (1: one block owns the tile), multi_mask bool [n, 7]: the (row, dir) slots that gather an aux row.

    Operands.  a = decode(planes) is what the reference contracts, so a direct row and a type row are exact.
      fp16 pairs (mode 3): the weight enters as (w s)_hi + (w s)_lo, s the pack's power of two (undone exactly in the
        epilogue): |dw| <= 2^-22 |w| + 2^-25 / s (gemm_oracle.bound: the same split, the tensor's own s and its denormal
        floor).  The product a w is evaluated as a_lo w_hi + a_hi w_lo + a_hi w_hi, dropping a_lo w_lo with
        |a_lo| <= 2^-11 |a| and |w_lo| <= 2^-11 |w|: 2^-22 |a w|.  Per term 2 * 2^-22 |a w| = 8 U |a w|, plus the floor
        (2^-25 / s) |a|:  c_op = 8, floor = (2^-25 / s) asum.
      bf16 pairs (mode 2): 8-bit halves, no scale, no floor: |dw| <= 2^-16 |w|, dropped lo lo <= 2^-16 |a w|:
        c_op = 2 * 2^-16 / U = 512.
      fp16 (mode 1): one rounding of w s to fp16, activations exact (they ARE fp16): |dw| <= 2^-11 |w| + 2^-25 / s:
        c_op = 2^-11 / U = 8192, floor = (2^-25 / s) asum.
    Aux rows.  A slot in multi_mask gathers the fp32 mean over its e - b sources, split into the mode's format again:
        |da| <= aux_err (above) for each of its cin channels, which enters the output as sum_c aux_err[c] |w[dir, c, n]|
        -- added for those slots only: r['aux_slot_err'] masked by multi_mask, times |W|.
    Accumulation.  Every fp16 / bf16 product is exact in fp32 and joins the fp32 accumulator with one rounding: depth
        3 chain in the pair modes, chain in mode 1; `pieces` partial sums added in k order; one fma for scale and bias, one
        add each for emb and res:  c_acc = (3 | 1) chain + pieces + 3, against S, which bounds every partial |sum|.
    (1 + 2^-10) covers the products of two of the errors above, 1 / (1 - c U) the compounding of the roundings."""
    S = r['S']
    s = weight_scale(r['wmax'])
    if mode == 3:
        c_op, floor, per = 8.0, (2.0 ** -25 / s) * r['asum'], 3
    elif mode == 2:
        c_op, floor, per = 512.0, 0.0, 3
    elif mode == 1:
        c_op, floor, per = 8192.0, (2.0 ** -25 / s) * r['asum'], 1
    else:
        raise ValueError(mode)
    c = c_op + per * chain + pieces + 3
    n = S.shape[0]
    E = r['aux_slot_err'] * multi_mask[:, :, None].double()
    aux_term = E.reshape(n, -1) @ r['Wabs']
    return (c * U * S + floor + aux_term) * (1.0 + 2.0 ** -10) / (1.0 - c * U)


STATS_DEPTH = {'float4': 11, 'scalar': 32}


def stats_sums(y, bid, B):
    """float64 [B, cout, 2]: sum and sum of squares of the STORED outputs per batch element, and their magnitudes"""
    yd = y.detach().cpu().double()
    s = torch.zeros(B, yd.shape[1], 2, dtype=torch.float64)
    s[:, :, 0].index_add_(0, bid.long(), yd)
    s[:, :, 1].index_add_(0, bid.long(), yd * yd)
    mag = torch.zeros(B, yd.shape[1], dtype=torch.float64)
    mag.index_add_(0, bid.long(), yd.abs())
    return s, mag


def stats_bound(y, bid, B, path):
    """(bS, bQ) float64 [B, cout]: admissible |stats - float64 sums of the stored y, y^2|.
    float4 epilogue: a lane adds its 8 rows of a wave serially in fp32, three butterfly steps add the 8 lanes that share a
        column (depth 8 + 3 = 11 for the 64 rows of a wave; a wave that holds two batch elements keeps two such sums, three or
        more: per-lane runs of <= 8), the per-wave fp32 sums are then added in fp64 (second-stage reducer or fp64 atomics).
    scalar epilogue: a lane owns one column and adds its 32 rows of the wave tile serially in fp32 (a run ends where the
        batch label changes), then one fp64 atomic per run: depth 32.
    A sum of depth D in fp32 is within D U sum|y| / (1 - D U); every square is rounded once more: (D + 1) U sum y^2.  The
    fp64 additions (at most one per wave and run, < 2^12 here) add 2^-53 each: 2^-41 of the same magnitudes."""
    D = STATS_DEPTH[path]
    s, mag = stats_sums(y, bid, B)
    bS = (D * U / (1 - D * U) + 2.0 ** -41) * mag
    bQ = ((D + 1) * U / (1 - (D + 1) * U) + 2.0 ** -41) * s[:, :, 1]
    return bS, bQ


# ------------------------------------------------------------------------------------------------ weight pack
def kernel_order(c_or_W, cin=None, nt=None, mode=None):
    """fp32 [nkt * chunk, cout]: the reference rows dir * (cin + ntc) + c in the pack's k order -- 7 cin gathered channels
    direction-major, then the 7 ntc type rows (dir * ntc + t), zero rows up to a whole tile."""
    if cin is None:
        W, cin, nt, mode = c_or_W.W, c_or_W.cin, c_or_W.nt, c_or_W.mode
    else:
        W = c_or_W
    t = ntc(nt)
    W3 = W.view(7, cin + t, -1)
    out = torch.zeros(ktiles(cin, nt, mode) * chunk(mode), W.shape[1])
    out[:7 * cin] = W3[:, :cin].reshape(7 * cin, W.shape[1])
    out[7 * cin:7 * cin + 7 * t] = W3[:, cin:].reshape(7 * t, W.shape[1])
    return out


def pack_scale(W, mode):
    """the per-tensor power of two of the fp16 formats (modes 1 and 3); bf16 pairs have fp32's exponent range: 1"""
    return 1.0 if mode == 2 else weight_scale(float(W.abs().max()))


def pack_reference(W, cin, nt, cout, mode):
    """uint8 [packed_bytes]: ofx_pack_weights_planes by the header -- [k tile][column][128-B line] of W s in the mode's
    format ([hi x 32 | lo x 32] or 64 fp16), then the trailer line whose first two floats are [1 / s, s] (the rest of the
    trailer is unspecified: compare packed[:-120])."""
    assert W.shape == (7 * (cin + ntc(nt)), cout)
    s = pack_scale(W, mode)
    Ws = kernel_order(W.float(), cin, nt, mode) * s
    nkt = ktiles(cin, nt, mode)
    lines = GN.encode(Ws.t().contiguous(), mode).view(cout, nkt, LINE).permute(1, 0, 2).reshape(-1)
    trailer = torch.zeros(LINE // 4)
    trailer[0], trailer[1] = 1.0 / s, s
    return torch.cat([lines, trailer.view(torch.uint8)])


def pack_decode(raw, cin, nt, cout, mode):
    """float64 [nkt * chunk, cout]: the values a pack holds (W s in kernel order)"""
    nkt = ktiles(cin, nt, mode)
    lines = raw[:nkt * cout * LINE].view(nkt, cout, LINE).permute(1, 0, 2).reshape(cout, nkt * LINE)
    return GN.decode(lines, nkt * chunk(mode), mode).t()


# ------------------------------------------------------------------------------------------------ host emulation
MUTATIONS = ('drop_alo_whi', 'drop_ahi_wlo', 'drop_dir', 'swap_type_dirs', 'wrong_count', 'aux_for_zero', 'emb_next',
             'keep_scale', 'lo_hi')


def applies(mut, c):
    """the shapes a planted error can show on"""
    if mut in ('drop_alo_whi', 'drop_ahi_wlo', 'lo_hi'):
        return pairs(c.mode) and c.probe is not None
    if mut == 'swap_type_dirs':
        return c.ntc > 0
    if mut == 'wrong_count':
        return len(c.multi) > 0
    if mut == 'aux_for_zero':
        return len(c.multi) > 0 and bool((c.ext == c.n).any())
    if mut == 'emb_next':
        return c.B > 1
    if mut == 'keep_scale':
        return pack_scale(c.W, c.mode) != 1.0
    return True


def _cast(t, mode):
    return t.bfloat16().float() if mode == 2 else t.half().float()


def emulate(c, pieces=1, mut=None):
    """fp32 [n, cout]: an honest implementation on the host -- aux rows summed serially in fp32, times the rounded 1 / L,
    re-split; operands split into the mode's halves; per k tile the three products (one in mode 1) added to an fp32
    accumulator; `pieces` runs of tiles added in k order; scale undone and bias added by one fma, emb and res added.
    `mut`: one of MUTATIONS, the planted errors of tests/test_gconv_planes_oracle.py."""
    mode, n, cin = c.mode, c.n, c.cin
    ch = chunk(mode)
    xq = c.xd.float()                                  # decoded values are fp32 numbers
    src, L = _seg_sources(c)
    a32 = torch.zeros(len(L) + 1, cin)
    if len(L):
        acc = torch.zeros(len(L), cin)
        for p in range(src.shape[1]):
            acc = acc + xq[src[:, p]] * (p < L)[:, None].float()
        cnt = L.float() + (1.0 if mut == 'wrong_count' else 0.0)
        a32[1:] = acc * (torch.ones(len(L)) / cnt)[:, None]
    auxq = GN.decode(GN.encode(a32, mode), cin, mode).float()
    tab = c.ext.long().clone()
    if mut == 'aux_for_zero':
        tab[tab == n] = n + 1
    rows = torch.cat([xq, auxq])[tab]                  # [n, 7, cin]
    if mut == 'drop_dir':
        rows[:, 3] = 0.0
    tf = c.tfd.float().view(n, 7, c.ntc)
    if mut == 'swap_type_dirs':
        tf = tf[:, [1, 0, 2, 3, 4, 5, 6]]
    A = torch.zeros(n, c.nkt * ch)
    A[:, :7 * cin] = rows.reshape(n, 7 * cin)
    A[:, 7 * cin:7 * cin + 7 * c.ntc] = tf.reshape(n, 7 * c.ntc)
    s = pack_scale(c.W, mode)
    Ws = kernel_order(c) * s
    wh = _cast(Ws, mode)
    if pairs(mode):
        wl = _cast(Ws - wh, mode)
        ah = _cast(A, mode)
        al = _cast(A - ah, mode)
        if mut == 'lo_hi':                             # the pack wrote [lo | hi]: the kernel takes lo for hi
            wh, wl = wl, wh
    edges = [round(i * c.nkt / pieces) for i in range(pieces + 1)]
    total = None
    for i in range(pieces):
        acc = torch.zeros(n, c.cout)
        for t in range(edges[i], edges[i + 1]):
            k = slice(t * ch, (t + 1) * ch)
            if pairs(mode):
                if mut != 'drop_alo_whi':
                    acc = acc + al[:, k] @ wh[k]
                if mut != 'drop_ahi_wlo':
                    acc = acc + ah[:, k] @ wl[k]
                acc = acc + ah[:, k] @ wh[k]
            else:
                acc = acc + A[:, k] @ wh[k]
        total = acc if total is None else total + acc
    osc = torch.tensor(1.0 if mut == 'keep_scale' else 1.0 / s)
    out = GM._fma32(c.bias.float().expand(n, c.cout), total, osc)
    bid = (c.bid.long() + (1 if mut == 'emb_next' else 0)) % c.B
    return out + c.emb.float()[bid] + c.res.float()


# ------------------------------------------------------------------------------------------------ persistent plan
def plan_pieces(plan, nkt):
    """Most partial sums any tile of the stream-K region is cut into: plan = the int32 words ofx_gconv3_plan wrote
    (out[0] = G, out[5 .. 5 + G] = share boundaries in k-step units from the region's start)."""
    G = int(plan[0])
    cuts = [int(b) for b in plan[5:5 + G + 1]]
    inside = {}
    for b in cuts[1:-1]:
        if b % nkt:
            inside[b // nkt] = inside.get(b // nkt, 0) + 1
    return 1 + max(inside.values(), default=0), bool(inside)


# ------------------------------------------------------------------------------------------------ shared shape tables
def cin_for(cin, mode):
    """mode 1 lines hold 64 channels: the 32-channel shapes run at 64 there"""
    return max(cin, 64) if mode == 1 else cin


# rows: the last 128-row tile, the last 256-row tile and the last 64-row wave are all partial; more than one block
#                 name        n   cin nt cout
SCALAR_WIDTHS = [('cout3', 331, 32, 4, 3), ('cout70', 459, 64, 0, 70), ('cout130', 587, 128, 5, 130)]
TRIGGER_SHAPE = ('cout128', 395, 64, 4, 128)
TRIGGERS = ('ldc', 'out', 'res', 'ldr', 'lde', 'bias')            # each alone sends cout = 128 to the scalar epilogue
LABEL_SHAPE = ('labels', 451, 64, 4, 70)
# one, two and three or more batch elements inside a 64-row wave, a boundary on a wave boundary, a 3-row tail
LABEL_CUTS = [0, 100, 110, 192, 300, 451 - 3, 451]
PITCH_SHAPE = ('pitch', 363, 64, 9, 72)                            # 7 * 9 = 63 type rows: two 32-channel tiles
# 3 column tiles: enough k-step units for >= 8 persistent blocks; nt = 10: 70 type rows cross a k tile in every mode, and
# mode 1 gets 16 k-steps per tile -- the fewest that a share boundary can cut (a piece has >= 8)
LADDER_SHAPE = ('ladder', 587, 128, 10, 384)
AUX_SHAPES = [('multi289', 301, 64, 2, 64, (0, 1, 2, 8, 9, 2)), ('nomulti', 301, 64, 2, 64, (0, 1, 1, 1, 0, 1))]
PACK_NTS = (0, 1, 2, 4, 5, 9, 10)
ALL_SHAPES = SCALAR_WIDTHS + [TRIGGER_SHAPE, LABEL_SHAPE, PITCH_SHAPE, LADDER_SHAPE] + AUX_SHAPES

_CASES = {}


def case(shape, mode, sizes=(0, 1, 2, 8, 9, 3), cuts=None):
    """make_case of a table row, built once per (row, mode) and left unchanged"""
    name, n, cin, nt, cout = shape[:5]
    sizes = shape[5] if len(shape) > 5 else sizes
    key = (name, mode, sizes, tuple(cuts) if cuts else None)
    if key not in _CASES:
        _CASES[key] = make_case(n, cin_for(cin, mode), nt, cout, mode, 7 * n + cout + 1000 * mode, sizes, cuts)
    return _CASES[key]
