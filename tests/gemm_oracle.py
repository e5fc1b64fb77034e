"""float64 torch restatement of the GEMM core (ofx_gemm_f32, ofx_gemm_f32_planes, ofx_gather_gemm_f32), written from the
formulas of include/ofx.h ("GEMM core", ofx_gather_gemm_f32, the precision-mode and range-guard comments), with ONE
elementwise error bound per contraction flavour, the host emulations that show those bounds admit an honest
implementation, a mirror of the launcher's tiling arithmetic, and the shape tables the CPU and GPU tests share.  Nothing
here imports octfusion_amd.

Every reference returns the float64 result and, per element, the MAGNITUDE S = sum_k |a_k| |w_k| + |bias| + |res|.
`bound` turns S into the largest |got - ref| the flavour may show; the bound of one element depends on that element's own
operands only (its row of A, its column of W, max|w| of the tensor through the pack's scale), never on another output.
A dropped or misplaced term is off by about S / K -- far above any of the bounds below.
"""
import math
from collections import namedtuple

import torch

U = 2.0 ** -24            # unit roundoff of fp32
BM, BK = 128, 32
WS_DEFAULT = 96 << 20     # ops.workspace


def pad32(v):
    return (v + 31) // 32 * 32


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------ launcher decisions
Plan = namedtuple('Plan', 'bn ntm ntn nsplit kt_per_split')


def plan(M, N, K, ws_bytes=WS_DEFAULT, ws=True):
    """(bn, ntm, ntn, nsplit, kt_per_split) of a launch: column tile by N, split-K when the tile grid is below 256 tiles
    and there are >= 8 k tiles -- 512 blocks aimed for, >= 4 k tiles per slice, <= 64 slices, no more slices than the
    workspace holds partials [M, N] for (fewer than two: a single pass); the slice count is then re-derived from the
    rounded-up tiles per slice, so the last slice may be shorter.  K is the logical K (Kp = pad32(K) is contracted)."""
    bn = 32 if N <= 32 else (64 if N <= 64 else 128)
    ntm, ntn = cdiv(M, BM), cdiv(N, bn)
    nkt = pad32(K) // BK
    nsplit, tiles = 1, ntm * ntn
    if ws and tiles < 256 and nkt >= 8:
        nsplit = min(cdiv(512, tiles), nkt // 4, 64)
        per = M * N * 4
        if nsplit * per > ws_bytes:
            nsplit = ws_bytes // per
        if nsplit < 2:
            nsplit = 1
    kps = cdiv(nkt, nsplit)
    return Plan(bn, ntm, ntn, cdiv(nkt, kps), kps)


def flavour(precision, K, lda, a_off_bytes=0, gather=False):
    """Kernel flavour: 'generic' (bounds-checked exact fp32: dense rows the branch-free loader cannot take -- K % 4, K < 4,
    lda % 4 or an A that is not 16-B aligned), else by precision: 1 -> 'fp32', 3 -> 'fp16x3', 0 / 2 -> 'bf16x3'."""
    if not gather and (K % 4 or K < 4 or lda % 4 or a_off_bytes % 16):
        return 'generic'
    return {1: 'fp32', 3: 'fp16x3'}.get(precision, 'bf16x3')


def kind_of(flav):
    """The bound that goes with a flavour."""
    return 'exact' if flav in ('generic', 'fp32') else flav


def vec4(N, ldc, out_off_bytes=0, res=False, ldr=0, res_off_bytes=0, bias_off_bytes=0):
    """float4 epilogue / reducer: N % 4 == 0 and out, res, bias 16-B aligned with pitches % 4 == 0."""
    return (N % 4 == 0 and ldc % 4 == 0 and out_off_bytes % 16 == 0 and bias_off_bytes % 16 == 0 and
            (not res or (ldr % 4 == 0 and res_off_bytes % 16 == 0)))


def reducer_loops(nsplit):
    """(runs of the 8-slice loop, of the 4-slice loop, of the 1-slice loop) of the float4 reducer."""
    return nsplit // 8, (nsplit % 8) // 4, nsplit % 4


def cell(precision, M, N, K, lda, ldc, a_off=0, out_off=0, res=False, ldr=0, res_off=0, ws_bytes=WS_DEFAULT, ws=True,
         gather=False):
    """(flavour, bn, epilogue, reducer, nsplit): the coverage cell of a case."""
    p = plan(M, N, K, ws_bytes, ws)
    v4 = vec4(N, ldc, out_off, res, ldr, res_off)
    red = 'none' if p.nsplit == 1 else ('float4' if v4 else 'scalar')
    epi = 'partials' if p.nsplit > 1 else ('float4' if v4 else 'scalar')
    return flavour(precision, K, lda, a_off, gather), p.bn, epi, red, p.nsplit


def chain_len(K, p):
    """Longest accumulation chain of one output element: the k terms of one slice (all of Kp without split-K)."""
    return min(pad32(K), p.kt_per_split * BK)


# ------------------------------------------------------------------------------------------------ references
def _contract(rows, W, bias, res, out_rows, n_out_rows):
    """rows: the float64 [M, K] operand rows in launch order.  See gemm()."""
    M = rows.shape[0]
    Wd = W.double()
    N = Wd.shape[1]
    val = rows @ Wd
    S = rows.abs() @ Wd.abs()
    if bias is not None:
        val = val + bias.double()
        S = S + bias.double().abs()
    if res is not None:
        val = val + res.double()[:M]
        S = S + res.double()[:M].abs()
    asum = rows.abs().sum(1, keepdim=True).expand(M, N)
    if out_rows is None:
        n_out_rows = M if n_out_rows is None else n_out_rows
        dst = torch.arange(M)
        keep = torch.ones(M, dtype=torch.bool)
    else:
        dst = out_rows.long()
        keep = dst >= 0
    ref = torch.zeros(n_out_rows, N, dtype=torch.float64)
    Sd = torch.zeros_like(ref)
    ad = torch.zeros_like(ref)
    written = torch.zeros(n_out_rows, dtype=torch.bool)
    ref[dst[keep]] = val[keep]
    Sd[dst[keep]] = S[keep]
    ad[dst[keep]] = asum[keep]
    written[dst[keep]] = True
    return dict(ref=ref, S=Sd, written=written, asum=ad, wsum=Wd.abs().sum(0, keepdim=True),
                wmax=float(Wd.abs().max()) if Wd.numel() else 0.0)


def gemm(A, W, bias=None, res=None, a_rows=None, out_rows=None, n_out_rows=None, m=None, full=False):
    """ofx.h: out[orow(m), n] = sum_k A[arow(m), k] W[k, n] + bias[n] + res[m, n]; a negative out_rows entry skips the row.
    W is [K, N].  Returns (ref, S, written): ref / S float64 [n_out_rows, N] (zero in rows nothing is written to),
    written the boolean mask of the destination rows some out_rows entry names.  full=True: a dict that also has the
    operand sums the floor terms of `bound` need (asum [rows, N] = sum_k |a_k|, wsum [1, N] = sum_k |w_k|, wmax)."""
    Ad = A.double()
    if a_rows is not None:
        Ad = Ad[a_rows.long()]
    if m is not None:
        Ad = Ad[:m]
        out_rows = out_rows[:m] if out_rows is not None else None
    r = _contract(Ad, W, bias, res, out_rows, n_out_rows)
    return r if full else (r['ref'], r['S'], r['written'])


def gather_rows(x, tab):
    """[n_out, ntap * cin] float64: row r = [x[tab[r, 0]] | ... | x[tab[r, ntap - 1]]]; an entry == n_src is a zero row."""
    xd = torch.cat([x.double(), torch.zeros(1, x.shape[1], dtype=torch.float64)])
    return xd[tab.long()].reshape(tab.shape[0], -1)


def gather_gemm(x, tab, W, bias=None, res=None, out_rows=None, n_out_rows=None, full=False):
    """ofx.h: out[orow(r), :] = [x[tab[r, 0], :] | ... | x[tab[r, ntap - 1], :]] @ W + bias + res[r], entries in
    [0, n_src] with n_src = x.shape[0] naming the zero row.  Returns as gemm()."""
    r = _contract(gather_rows(x, tab), W, bias, res, out_rows, n_out_rows)
    return r if full else (r['ref'], r['S'], r['written'])


# ------------------------------------------------------------------------------------------------ the bound
def weight_scale(wmax):
    """The per-tensor power of two s of the fp16 pack: max|w| * s lies in [2^14, 2^15) (ofx.h, range guard)."""
    if not wmax > 0.0:
        return 1.0
    _, e = math.frexp(float(torch.tensor(wmax, dtype=torch.float32)))      # wmax = f * 2^e, f in [0.5, 1)
    return 2.0 ** max(-60, min(60, 15 - e))


def bound(kind, r, chain, nsplit, out_planes=0):
    """Largest admissible |got - ref| per element (float64 tensor shaped like r['ref']); r = gemm(..., full=True).

    Common part -- what every flavour does after its products: each output is a chain of `chain` terms accumulated in
    fp32 (the k terms of one slice), `nsplit` partials added in slice order, one fma that adds the bias and one add of
    the residual.  A sum of depth D evaluated in fp32 is within D U sum|terms| / (1 - D U) of the exact sum
    (U = 2^-24); every |term| sum here is <= S.

    exact (precision 1; the generic flavour in every precision -- it reads the fp32 pack, no scale): one rounding per fma
        c = chain + nsplit + 2.
    fp16x3 (precision 3): a = a_hi + a_lo and w s = w_hi + w_lo in fp16 (11 bits each; s the pack's power of two, undone
        exactly in the epilogue), a w ~ a_lo w_hi + a_hi w_lo + a_hi w_hi.
          operand error: hi is within 2^-11 |a| of a and a - hi is exact in fp32; lo rounds it to 11 bits, or to a multiple
          of 2^-24 when it is an fp16 denormal (|a - hi| < 2^-14, which |a| < 2^-3 guarantees):
              |da| <= 2^-22 |a| + 2^-25;    |dw| <= 2^-22 |w| + 2^-25 / s    (the same on w s, divided by s).
          ofx.h states the weight floor as 2^-40 max|w|: max|w| s lies in [2^14, 2^15), so 2^-25 / s is between 2^-40 and
          2^-39 max|w| -- the header's figure is the upper end of the scale window; this bound takes the tensor's own s
          (weight_scale), which is what the pack uses.
          dropped a_lo w_lo: |a_lo| <= 2^-11 |a|, |w_lo| <= 2^-11 |w|: 2^-22 |a w|.
          per term: 3 * 2^-22 |a w| + 2^-25 |w| + (2^-25 / s) |a|  (+ products of two of these: the 1 + 2^-10 below);
          summed over k: 12 U S + 2^-25 sum_k |w_k| + (2^-25 / s) sum_k |a_k|.
          accumulation: every one of the three fp16 products of a term is exact in fp32 and enters the fp32 accumulator
          with at most one rounding: depth 3 * chain.
        c = 12 + 3 chain + nsplit + 2, plus the two floor sums.
    bf16x3 (precision 0; the dense GEMM under precision 2): the same with bf16 halves (8 bits each, fp32's exponent range:
        no scale, no denormal floor): |da| <= 2^-16 |a|, |dw| <= 2^-16 |w|, dropped lo lo <= 2^-16 |a w|:
        3 * 2^-16 = 768 U per term;  c = 768 + 3 chain + nsplit + 2.
    Pair-plane outputs (out_planes 3 / 2): the value v that would have been stored is split once more:
        + 2^-22 |v| + 2^-25 (fp16 pairs: the lo half of |v| < 2^-3 is a denormal) or 2^-16 |v| (bf16 pairs), |v| <= |ref| +
        the bound so far; + U |ref| for the hi + lo addition of the read-back.
    """
    S, ref = r['S'], r['ref']
    epi = nsplit + 2
    if kind == 'exact':
        c, floor = chain + epi, 0.0
    elif kind == 'fp16x3':
        c = 12.0 + 3 * chain + epi
        floor = 2.0 ** -25 * r['wsum'] + (2.0 ** -25 / weight_scale(r['wmax'])) * r['asum']
    elif kind == 'bf16x3':
        c, floor = 768.0 + 3 * chain + epi, 0.0
    else:
        raise ValueError(kind)
    b = (c * U * S + floor) * (1.0 + 2.0 ** -10) / (1.0 - c * U)
    if out_planes:
        rnd, pfloor = {3: (2.0 ** -22, 2.0 ** -25), 2: (2.0 ** -16, 0.0)}[out_planes]
        b = b + rnd * (ref.abs() + b) + pfloor + U * ref.abs()
    return b


def assert_close(got, ref, S, bnd, what='', rows=None):
    """|got - ref| <= bnd for every element (of the rows in the boolean mask `rows`, when given); NaN / inf in `got` fails.
    Reports the worst element with its (m, n) and its ratio to the bound; returns the largest ratio."""
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    bnd = torch.as_tensor(bnd, dtype=torch.float64).expand_as(ref)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    if rows is not None:
        got, ref, bnd, S = got[rows], ref[rows], bnd[rows], torch.as_tensor(S).expand_as(bnd)[rows]
        idx = torch.nonzero(rows).reshape(-1)
    else:
        idx = torch.arange(got.shape[0])
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd.clamp(min=1e-300))
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float('inf')))
    worst = int(ratio.reshape(-1).argmax())
    m, n = worst // got.shape[1], worst % got.shape[1]
    w = float(ratio[m, n])
    if not w <= 1.0:
        bad = int((~(ratio <= 1.0)).sum())
        raise AssertionError('%s: %d of %d elements off; worst (m, n) = (%d, %d): got %r ref %r |err| %.3e bound %.3e '
                             '(%.2f x the bound, S = %.3e)' % (what, bad, ratio.numel(), int(idx[m]), n, float(got[m, n]),
                                                               float(ref[m, n]), float(err[m, n]), float(bnd[m, n]), w,
                                                               float(torch.as_tensor(S).expand_as(bnd)[m, n])))
    return w


# ------------------------------------------------------------------------------------------------ host emulations
def _slices(K, p):
    Kp = pad32(K)
    step = p.kt_per_split * BK
    return [(k0, min(k0 + step, Kp)) for k0 in range(0, Kp, step)][:p.nsplit]


def _fma32(acc, a, w):
    """fp32 fma of [M, 1] x [1, N] into acc: the product of two fp32 is exact in fp64."""
    return (acc.double() + a.double() * w.double()).float()


def emulate(kind, rows, W, bias, res, p, drop_k=None, drop_slice=None, drop_lo=None, keep_scale=False):
    """fp32 [M, N]: the contraction as a kernel of `kind` evaluates it, on the host.  rows [M, K] fp32 in launch order.
    exact: an fma chain in k order per slice; fp16x3 / bf16x3: operands split with .half() / .bfloat16(), three products
    per term, each added to an fp32 accumulator; then the slices are added in slice order, the scale undone, bias added
    by fma, res added.  The planted errors of tests/test_gemm_oracle.py: drop_k (k values whose term is skipped),
    drop_slice (a slice the reduction leaves out), drop_lo ((m, k): that activation enters with its hi half only),
    keep_scale (the power-of-two weight scale is not undone)."""
    rows, W = rows.float(), W.float()
    M, K = rows.shape
    N = W.shape[1]
    drop_k = set(drop_k or ())
    s = 1.0
    if kind != 'exact':
        cast = (lambda t: t.half().float()) if kind == 'fp16x3' else (lambda t: t.bfloat16().float())
        if kind == 'fp16x3':
            s = weight_scale(float(W.abs().max()))
        ah = cast(rows)
        al = cast(rows - ah)
        if drop_lo is not None:
            al[drop_lo[0], drop_lo[1]] = 0.0
        ws = (W * s).clamp(-65504.0, 65504.0) if kind == 'fp16x3' else W
        wh = cast(ws)
        wl = cast(ws - wh)
    total = torch.zeros(M, N)
    for si, (k0, k1) in enumerate(_slices(K, p)):
        acc = torch.zeros(M, N)
        for k in range(k0, min(k1, K)):              # (k >= K: zero-padded weight rows, exact zeros)
            if k in drop_k:
                continue
            if kind == 'exact':
                acc = _fma32(acc, rows[:, k:k + 1], W[k:k + 1])
            else:
                acc = acc + al[:, k:k + 1] * wh[k:k + 1]
                acc = acc + ah[:, k:k + 1] * wl[k:k + 1]
                acc = acc + ah[:, k:k + 1] * wh[k:k + 1]
        if si != drop_slice:
            total = acc if p.nsplit == 1 else total + acc
    osc = 1.0 if keep_scale else 1.0 / s
    if bias is not None:
        total = _fma32(bias.float().expand(M, N), total, torch.tensor(osc))
    else:
        total = total * osc
    if res is not None:
        total = total + res.float()[:M]
    return total


def store_planes(v, mode):
    """fp32 -> what a pair-plane store (mode 3: fp16 pairs, 2: bf16 pairs) and the read-back hi + lo return."""
    cast = (lambda t: t.half().float()) if mode == 3 else (lambda t: t.bfloat16().float())
    hi = cast(v)
    return hi + cast(v - hi)


# ------------------------------------------------------------------------------------------------ inputs
def operand(shape, seed, scale=1.0):
    """Seeded randn * scale with a deterministic sprinkling of exact zeros (every 7th element), 1e-3 (every 11th) and
    50 (every 13th); everything stays far inside +-65504."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(*shape, generator=g) * scale
    f = t.reshape(-1)
    i = torch.arange(f.numel())
    f[i % 7 == 3] = 0.0
    f[i % 11 == 5] = 1e-3
    f[i % 13 == 6] = 50.0
    return t


def weight(K, N, seed, how='unit'):
    """[K, N]: 'unit' randn / sqrt(K) with the sprinkling; 'small' at 1e-4 scale; 'large' at 1e3; 'decades': magnitudes
    spread over six decades (10^-5 .. 10^1) with random signs."""
    g = torch.Generator().manual_seed(seed)
    if how == 'decades':
        mag = 10.0 ** (torch.rand(K, N, generator=g) * 6.0 - 5.0)
        return mag * torch.where(torch.rand(K, N, generator=g) < 0.5, -1.0, 1.0)
    w = torch.randn(K, N, generator=g) / math.sqrt(K)
    if how == 'plain':
        return w
    if how == 'unit':
        f = w.reshape(-1)
        i = torch.arange(f.numel())
        f[i % 7 == 2] = 0.0
        f[i % 13 == 4] = 1e-3
        f[i % 17 == 9] = 50.0
        return w
    return w * {'small': 1e-4, 'large': 1e3}[how]


def gather_table(n_out, ntap, n_src, g, how='random'):
    """int32 [n_out, ntap]: 'random' entries in [0, n_src] with every 5th entry the zero row (n_src) and every 9th ROW
    made of zero-row entries only; 'children': tab[r, j] = ntap * r + j (Downsample)."""
    if how == 'children':
        return torch.arange(n_out * ntap, dtype=torch.int32).reshape(n_out, ntap)
    tab = torch.randint(0, n_src + 1, (n_out, ntap), generator=g, dtype=torch.int32)
    f = tab.reshape(-1)
    f[torch.arange(f.numel()) % 5 == 2] = n_src
    tab[8::9] = n_src
    return tab


def gather_cout(cin, ntap, n_out):
    """Output width of a gather case: all three column tiles, one width with N % 4 != 0."""
    return (32, 64, 132, 36, 33, 260)[(cin // 32 + ntap + n_out) % 6]


def check_window(buf, row0, N, r, bnd, sentinel, what=''):
    """`buf`: host copy of a sentinel-filled [row0 + rows + pad, ldc] buffer whose rows row0.. and columns 0..N-1 are the
    destination.  Rows in r['written'] must be within `bnd` of r['ref']; everything else -- the pad rows, the columns
    right of N, every row no out_rows entry names -- bit-equal to the sentinel.  Returns the largest ratio to the bound."""
    R = r['ref'].shape[0]
    keep = torch.ones(buf.shape, dtype=torch.bool)
    keep[row0:row0 + R, :N] = ~r['written'][:, None]
    same = buf.contiguous().view(torch.int32) == torch.full_like(buf, sentinel).view(torch.int32)
    if not bool(same[keep].all()):
        i, j = [int(v) for v in torch.nonzero(keep & ~same)[0]]
        raise AssertionError('%s: %d elements outside the written rows / columns are not untouched; first at buffer row '
                             '%d (destination row %d), column %d: %r' % (what, int((keep & ~same).sum()), i, i - row0, j,
                                                                         float(buf[i, j])))
    return assert_close(buf[row0:row0 + R, :N], r['ref'], r['S'], bnd, what, rows=r['written'])


# ------------------------------------------------------------------------------------------------ shared shape tables
TILE_MS = (1, 127, 128, 129, 257)
TILE_NS = (1, 5, 32, 33, 64, 65, 130, 260)
TILE_KS = (4, 36, 96, 100)
# (M, N, K, packing, weight kind): every M and every K with every bn (N picks bn: <= 32, <= 64, else 128)
TILE_CASES = [(M, N, TILE_KS[(i + j) % 4], 'kn' if (i + j // 2) % 2 == 0 else 'nk',
               ('unit', 'small', 'decades', 'large')[(i + 2 * j) % 4])
              for i, N in enumerate(TILE_NS) for j, M in enumerate(TILE_MS)]
GENERIC_KS = (1, 3, 7, 30)
# split-K: (M, N, K); N = 36 the float4 reducer, 35 the scalar one
SPLITK_KS = (256, 512, 1664, 1696)
SPLITK_CASES = [(130, N, K) for N in (36, 35) for K in SPLITK_KS]
GATHER_CASES = [(cin, ntap, n_out) for cin in (32, 64) for ntap in (1, 8, 27) for n_out in (1, 129, 300)]
PRECISIONS = (1, 0, 3)
