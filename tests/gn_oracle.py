"""float64 torch restatement of the GroupNorm forward family of csrc/ofx_norm.hip (ofx_gn_stats / _acc, ofx_gn_finalize
/ _window, ofx_gn_apply, ofx_gn_apply_planes without a plan, ofx_gn_fused_rows), written from the arithmetic stated at the
top of ofx_norm.hip and in include/ofx.h, the independent decoders of the operand planes, the bound constants, and the
inputs and cases that tests/test_gn_oracle.py (host) and tests/test_gpu_gn_entry.py (device) share.  Nothing here imports
octfusion_amd; activations, their magnitudes and Lipschitz factors and the comparison helper are glue_oracle's.

Every comparison is glue_oracle.assert_close: |got - ref| <= c * 2^-24 * S elementwise, S the sum of the absolute values
of the terms that form the element, c derived next to the formula it belongs to (a number, or a tensor where the
conditioning differs per element).  All functions take `dtype`: with torch.float32 they are an honest fp32 evaluation on
the host, which tests/test_gn_oracle.py requires to pass the bounds the GPU tests use.
"""
import torch

import glue_oracle as G
from glue_oracle import U, assert_close          # noqa: F401  (the one comparison helper)

U64 = 2.0 ** -53
EPS = 1e-5
ACT_ID = {None: 0, 'silu': 1, 'gelu': 2}
STATS_ROWS = 64                                   # rows per statistics block unless a case says otherwise


def f32(v):
    """the float32 rounding of a Python number, as a Python float (what a `float` argument of the C ABI carries)"""
    return float(torch.tensor(v, dtype=torch.float32))


def layout(sizes):
    """non-decreasing int32 batch ids of elements with sizes[b] rows each"""
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.long)).to(torch.int32)


def make_x(sizes, C, groups, seed):
    """(x [n, C] float32, bid): per (batch element, group) a mean in [-2, 2] and a standard deviation in [0.25, 4];
    group 0 of the first non-empty element is the constant 1.7f (variance exactly 0), the last group of the last
    non-empty element lives at 1e-3 scale (mean and deviation)."""
    g = torch.Generator().manual_seed(seed)
    B, n, cpg = len(sizes), sum(sizes), C // groups
    bid = layout(sizes)
    mu = torch.rand(B, groups, generator=g, dtype=torch.float64) * 4 - 2
    sd = torch.rand(B, groups, generator=g, dtype=torch.float64) * 3.75 + 0.25
    z = torch.randn(n, C, generator=g, dtype=torch.float64)
    full = [b for b in range(B) if sizes[b] > 0]
    if len(full) * groups >= 2:                       # (a tensor that is one group keeps an ordinary one)
        mu[full[0], 0], sd[full[0], 0] = 1.7, 0.0
    if len(full) * groups >= 3:
        mu[full[-1], -1] *= 1e-3
        sd[full[-1], -1] *= 1e-3
    x = mu[bid.long()].repeat_interleave(cpg, 1) + sd[bid.long()].repeat_interleave(cpg, 1) * z
    return x.float(), bid


def make_affine(C, seed):
    g = torch.Generator().manual_seed(seed + 77)
    return (torch.rand(C, generator=g) + 0.5) * (1 - 2 * (torch.arange(C) % 3 == 1).float()), torch.randn(C, generator=g)


# ------------------------------------------------------------------------------------------------ statistics
def stats_run(C, rows_per_block=STATS_ROWS):
    """rows one thread of gn_stats_kernel sums in fp32: a block of `rows_per_block` rows is walked 256 / (C / 4) rows
    per pass, thread (row lane, float4) taking one row of every pass"""
    return -(-rows_per_block // (256 // (C // 4)))


def sums(x, bid, B, dtype=torch.float64, run=1):
    """(s, mag) float64 [B, C, 2]: s = (sum x, sum x^2) per batch element and channel, mag = (sum |x|, sum x^2).
    dtype float32: runs of `run` consecutive rows of an element are summed serially in fp32 (one product, one sum per
    row), the runs in float64 -- the kernel's scheme."""
    C = x.shape[1]
    s = torch.zeros(B, C, 2, dtype=torch.float64)
    mag = torch.zeros(B, C, 2, dtype=torch.float64)
    xd = x.double()
    mag[:, :, 0].index_add_(0, bid.long(), xd.abs())
    mag[:, :, 1].index_add_(0, bid.long(), xd * xd)
    if dtype == torch.float64:
        s[:, :, 0].index_add_(0, bid.long(), xd)
        s[:, :, 1] = mag[:, :, 1]
        return s, mag
    for b in range(B):
        xb = x[bid == b].float()
        nb = xb.shape[0]
        if nb == 0:
            continue
        pad = -nb % run
        xb = torch.cat([xb, torch.zeros(pad, C)]).view(-1, run, C)
        a, q = torch.zeros(xb.shape[0], C), torch.zeros(xb.shape[0], C)
        for i in range(run):
            a = a + xb[:, i]
            q = q + xb[:, i] * xb[:, i]
        s[b, :, 0], s[b, :, 1] = a.double().sum(0), q.double().sum(0)
    return s, mag


def sums_c(run):
    """(c of sum x, c of sum x^2).  A serial fp32 sum of `run` terms is within (run - 1) U sum |terms| (first order);
    every product x x adds one rounding of its term; the conversions to fp64 are exact and everything after them (LDS
    reduction, atomics in any order, a pre-filled buffer) rounds at 2^-53, 2^29 times finer: one more unit covers it.
    run = 16 (C = 256), 64 (C = 1024): c = (16, 17), (64, 65); the 128-row block at C = 256: (32, 33); the 192-row block
    at C = 1024: (192, 193)."""
    return float(run), float(run + 1)


# ------------------------------------------------------------------------------------------------ finalize
def _cnt_inv(count, cpg, count_eps):
    cnt = count.float() * torch.tensor(float(cpg), dtype=torch.float32)             # fp32, as the reference forms it
    inv = torch.tensor(1.0, dtype=torch.float32) / (cnt + torch.tensor(count_eps, dtype=torch.float32))
    return cnt.double()[:, None], inv.double()[:, None]


def finalize(S, SS, count, C, groups, eps, count_eps, dtype=torch.float64):
    """(mean, rstd) [B, C] of the first C columns of S / SS [B, pitch] (a channel window of a wider statistics buffer is
    the slice S[:, c_lo:], its pitch the buffer's): cnt = count cpg and inv = 1 / (cnt + count_eps) rounded to fp32,
    m = S inv, var = max(SS - 2 m S + cnt m^2, 0) inv, rstd = 1 / sqrt(var + eps) in float64; dtype float32 rounds the
    two results, which is all the kernel does in fp32."""
    B, cpg = S.shape[0], C // groups
    Sg = S[:, :C].double().reshape(B, groups, cpg).sum(2)
    Qg = SS[:, :C].double().reshape(B, groups, cpg).sum(2)
    cnt, inv = _cnt_inv(count, cpg, count_eps)
    m = Sg * inv
    var = (Qg - 2.0 * m * Sg + cnt * m * m).clamp(min=0) * inv
    rstd = 1.0 / torch.sqrt(var + f32(eps))
    return m.repeat_interleave(cpg, 1).to(dtype), rstd.repeat_interleave(cpg, 1).to(dtype)


def stat_bounds(S, SS, magS, magQ, cS, cQ, unit, count, C, groups, eps, count_eps):
    """(dm, dr) [B, C]: the absolute error of the mean and the relative error of rstd that errors |dS| <= cS unit sum |x|,
    |dSS| <= cQ unit sum x^2 of the sums cause, to first order, BEFORE the two results are rounded to fp32:
      dm = dS inv;   ssd(S, SS) = SS - 2 inv S^2 + cnt inv^2 S^2, d ssd / dS = 2 m (cnt inv - 2):
      d ssd = dSS + 2 |m| |2 - cnt inv| dS + 4 2^-53 (SS + 2 |m S| + cnt m^2)   (the last: its own fp64 evaluation)
      d var = d ssd inv;   rstd = (var + eps)^-1/2:  dr = d var / (2 (var + eps)) -- the group's variance (+ eps) in the
    denominator: a quiet group amplifies, the constant group (var = 0) by 1 / (2 eps)."""
    B, cpg = S.shape[0], C // groups
    grp = lambda t: t[:, :C].double().reshape(B, groups, cpg).sum(2)
    Sg, Qg = grp(S), grp(SS)
    eS, eQ = cS * unit * grp(magS), cQ * unit * grp(magQ)
    cnt, inv = _cnt_inv(count, cpg, count_eps)
    m = Sg * inv
    var = (Qg - 2.0 * m * Sg + cnt * m * m).clamp(min=0) * inv
    dssd = eQ + 2.0 * m.abs() * (2.0 - cnt * inv).abs() * eS + 4.0 * U64 * (Qg + 2.0 * (m * Sg).abs() + cnt * m * m)
    dr = dssd * inv / (2.0 * (var + f32(eps)))
    return (eS * inv).repeat_interleave(cpg, 1), dr.repeat_interleave(cpg, 1)


def finalize_c(S, SS, count, C, groups, eps, count_eps):
    """(c of mean, c of rstd) against S = |mean| / rstd themselves for ofx_gn_finalize on GIVEN fp64 sums: the one fp32
    rounding of each result (1), plus stat_bounds at unit 2^-53 for the cpg + 3 fp64 operations in front of it -- about
    1e-6 of a unit for an ordinary group, 2e-3 for the constant one."""
    cpg = C // groups
    dm, dr = stat_bounds(S, SS, S.abs(), SS.abs(), cpg + 3.0, cpg + 3.0, U64, count, C, groups, eps, count_eps)
    m, _ = finalize(S, SS, count, C, groups, eps, count_eps)
    return 1.0 + dm / (U * m.abs().clamp(min=1e-300)), 1.0 + dr / U


# ------------------------------------------------------------------------------------------------ apply
def apply(x, bid, mean, rstd, w, b, act, dtype=torch.float64):
    """out = act((x - mean[bid]) rstd[bid] w + b).  Returns (ref, S, pre): S = |x - m| rstd |w| + |b|, pre = the value
    the activation is applied to."""
    i = bid.long()
    xx, m, r, ww, bb = x.to(dtype), mean.to(dtype)[i], rstd.to(dtype)[i], w.to(dtype), b.to(dtype)
    pre = (xx - m) * r * ww + bb
    S = (x.double() - mean.double()[i]).abs() * rstd.double()[i] * w.double().abs() + b.double().abs()
    return G.act(pre, act)[0], S, pre


ACT_OUT_C = {None: 0.0, 'silu': 10.5, 'gelu': 12.0}          # glue_oracle.linear_small_c: one evaluation of act on |v| <= S


def apply_c(x, bid, mean, rstd, w, S, act, dm, dr):
    """c (elementwise) of the normalised output against S.  Before the activation
      |d pre| <= (dm + U |m|) rstd |w|  +  |x - m| rstd |w| (dr + U)  +  4 U S:
    the mean's error and its rounding to fp32 (which |x - m| does not bound: where x is near the mean the term is what
    is left, so c grows there instead of S), rstd's error and rounding, and the apply's difference, two products and
    sum.  The activation multiplies that by its Lipschitz factor and adds its own evaluation (glue_oracle).  With exact
    sums, |m| <= 2, rstd |w| <= 6: c is 4 + 1 + U-units of |m| rstd |w| / S, some tens; with kernel sums it grows by
    cS / sqrt(rows) for an ordinary group."""
    i = bid.long()
    m, r, aw = mean.double()[i], rstd.double()[i], w.double().abs()
    A = (dm[i] + U * m.abs()) * r * aw + (x.double() - m).abs() * r * aw * (dr[i] + U) + 4.0 * U * S
    return A / (U * S.clamp(min=1e-300)) * G.LIPSCHITZ[act] + ACT_OUT_C[act]


# ------------------------------------------------------------------------------------------------ operand planes
def decode_pairs(raw, C, mode):
    """raw: uint8 [n, pitch in bytes] (host).  Modes 2 / 3: every 32-channel chunk is one 128-byte line
    [hi x 32 | lo x 32] of bf16 / fp16 halves; the value is hi + lo (float64: exact)."""
    n = raw.shape[0]
    half = raw[:, :C * 4].contiguous().view(torch.int16).view(torch.float16 if mode == 3 else torch.bfloat16)
    v = half.view(n, C // 32, 2, 32).double()
    return (v[:, :, 0] + v[:, :, 1]).reshape(n, C)


def decode_hi(raw, C, mode):
    """the hi halves alone (modes 2 / 3): what tells [hi | lo] from [lo | hi], which hi + lo cannot.  hi is the value
    rounded to its format: within HI_C U of it."""
    n = raw.shape[0]
    half = raw[:, :C * 4].contiguous().view(torch.int16).view(torch.float16 if mode == 3 else torch.bfloat16)
    return half.view(n, C // 32, 2, 32)[:, :, 0].double().reshape(n, C)


HI_C = {3: 2.0 ** 13, 2: 2.0 ** 16}               # 2^-11 (fp16) and 2^-8 (bf16) relative, in units of U (+ rep_c's 2^-25)


def decode_f16(raw, C):
    """mode 1: fp16 rows"""
    return raw[:, :C * 2].contiguous().view(torch.int16).view(torch.float16).double()


def decode(raw, C, mode):
    return decode_f16(raw, C) if mode == 1 else decode_pairs(raw, C, mode)


def encode(y, mode, pitch_bytes=None):
    """the same formats written on the host with torch's own conversions (round to nearest even): y float32 [n, C] ->
    uint8 [n, pitch]: what an honest kernel stores"""
    n, C = y.shape
    if mode == 1:
        raw = y.to(torch.float16).view(torch.int16)
    else:
        dt = torch.float16 if mode == 3 else torch.bfloat16
        hi = y.to(dt)
        lo = (y - hi.float()).to(dt)
        raw = torch.stack([hi.view(n, C // 32, 32), lo.view(n, C // 32, 32)], 2).reshape(n, 2 * C).view(torch.int16)
    raw = raw.contiguous().view(torch.uint8)
    if pitch_bytes and pitch_bytes > raw.shape[1]:
        raw = torch.cat([raw, torch.zeros(n, pitch_bytes - raw.shape[1], dtype=torch.uint8)], 1)
    return raw


def rep_c(mode, S):
    """what the representation adds to c (csrc/ofx_planes.h), against S >= |y|:
      mode 2, bf16 pairs: hi keeps 8 bits, lo the next 8: 2^-17 relative = 128 U;
      mode 3, fp16 pairs: 11 + 11 bits: 2^-23 relative = 2 U while lo is a normal fp16, half a subnormal step = 2^-25
              ABSOLUTE below: 2 + 2^-25 / (U S) = 2 + 0.5 / S covers both;
      mode 1, fp16: 2^-11 relative = 8192 U (and the same 2^-25 below the normal range)."""
    S = S.clamp(min=1e-300)
    if mode == 2:
        return torch.full_like(S, 128.0)
    return (2.0 if mode == 3 else 8192.0) + 0.5 / S


# ------------------------------------------------------------------------------------------------ aux rows
def aux_rows(y, seg_ptr, col, multi_seg, dtype=torch.float64):
    """[V + 1, C]: the zero row, then per multi-neighbour segment multi_seg[v] the mean of the normalised source rows
    y[col[seg_ptr[s] : seg_ptr[s + 1]]] (float32: summed serially, times the rounded 1 / length)."""
    out = torch.zeros(len(multi_seg) + 1, y.shape[1], dtype=dtype)
    for v, s in enumerate(multi_seg.tolist()):
        src = col[int(seg_ptr[s]):int(seg_ptr[s + 1])].long()
        acc = torch.zeros(y.shape[1], dtype=dtype)
        for r in src.tolist():
            acc = acc + y[r].to(dtype)
        out[v + 1] = acc * (torch.tensor(1.0, dtype=dtype) / torch.tensor(float(len(src)), dtype=dtype))
    return out


def aux_c(c_src, seg_ptr, col, multi_seg):
    """c of an aux row against S = the mean of its sources' S: the largest c among its sources (a mean of bounds
    c_i U S_i is at most max c_i times U mean S_i), the kernel's sum in groups of four -- 4 ceil(len / 4) additions,
    padded with zero terms --, the rounded 1 / len and the product with it (2).  The representation comes on top."""
    out = torch.zeros(len(multi_seg) + 1, c_src.shape[1], dtype=torch.float64)
    for v, s in enumerate(multi_seg.tolist()):
        src = col[int(seg_ptr[s]):int(seg_ptr[s + 1])].long()
        out[v + 1] = c_src[src].max(0)[0] + 4 * ((len(src) + 3) // 4) + 2
    return out


# ------------------------------------------------------------------------------------------------ fused rows
def fused_c(rows, cpg):
    """(cS, cQ) of the statistics inside ofx_gn_fused_rows, covering both kernels: one block per group sums
    ceil(rows cpg / 256) terms per thread serially in fp32; the 16-channel kernel adds a float4 as a depth-2 tree,
    accumulates ceil(rows / 256) of them and crosses four fp32 shuffle levels: depth ceil(rows / 256) + 6.  fp64 from
    there.  rows = 3073, cpg = 16: (193, 194); rows = 2048, cpg = 2: (16, 17)."""
    d = max(-(-rows * cpg // 256), -(-rows // 256) + 6)
    return float(d), float(d + 1)


# ------------------------------------------------------------------------------------------------ shared cases
# statistics: (sizes per batch element); n in {0, 1, 63, 64, 65, 257} at B = 3 as (1, 0, n - 1): a one-row element, an
# empty one, and a boundary at row 1 -- inside the first row pass for every C but 1024; (101, 57, 99): boundaries inside
# a row pass (C <= 96: >= 10 rows per pass) and inside the four-loads-in-flight loop (C = 256: 16 rows per trip);
# seven elements inside one 64-row block
STATS_LAYOUTS = [(0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 0, 62), (1, 0, 63), (1, 0, 64), (1, 0, 256), (101, 57, 99),
                 (9, 9, 9, 9, 9, 9, 10)]
STATS_C = [4, 12, 20, 96, 100, 256, 516, 1024]
# (C, rows, rows per block): gn_stats_rows by hand --
#   n = 4097, C = 256, B = 1: 65 chunks of 64 rows; 4 195 328 bytes / 512 KB = 8 blocks per element -> cap max(8, 64) = 64
#     < 65: a block owns 64 ceil(65 / 64) = 128 rows, a thread 128 / 4 = 32 of them;
#   n = 8193, C = 1024, B = 1: 129 chunks; 33 558 528 bytes / 512 KB = 64 -> cap 64 < 129: 64 ceil(129 / 64) = 192 rows per
#     block, one row per pass: a thread sums 192 rows in fp32.
STATS_BIG = [(256, 4097, 128), (1024, 8193, 192)]

# fp32 apply: C -> channels per group; layouts with n in {1, 63, 65, 200}: three elements inside one block (the middle
# one is neither the block's first nor its last row's: the fallback), seven inside one block, an empty element
APPLY_CPG = {4: (1, 2, 4), 8: (1, 2, 4), 12: (1, 2, 3, 4, 6), 96: (1, 2, 3, 4, 6), 100: (1, 2, 4), 1024: (1, 2, 4)}
APPLY_LAYOUTS = [(1,), (21, 20, 22), (9, 9, 9, 9, 9, 9, 11), (70, 0, 60, 70)]
PLANES_CASES = [(m, C) for m in (2, 3) for C in (32, 64, 96, 1024)] + [(1, 64), (1, 128)]
PLANES_LAYOUTS = [(21, 20, 22), (70, 0, 60, 70)]

# fused rows: (C, groups); rows on both sides of the 2048 threshold, with and without a remainder of the 1024-row trip
FUSED_ROWS = [2047, 2048, 2049, 2817, 3073]
FUSED_CASES = list(zip(FUSED_ROWS, (3, 3, 1, 1, 3)))          # (rows per batch element, B)
FUSED_WIDTHS = [(16, 1), (32, 16), (64, 16), (128, 16), (24, 12), (48, 8), (96, 8)]      # cpg 16 2 4 8 | 2 (G = 12) | 6 12


def aux_case():
    """130 rows, B = 2 (70 + 60), C = 64: (seg_ptr [7 n + 1], col, multi_seg, bid).  Segment s = 7 row + direction;
    18 multi-neighbour segments (19 aux rows: two aux blocks of 16 row lanes) with 2, 4, 5 and 9 sources in turn, the
    sources in the batch element of the segment's row, in both elements; every other segment has one source."""
    n, sizes = 130, (70, 60)
    bid = layout(sizes)
    lens = torch.ones(7 * n, dtype=torch.long)
    rows = [3, 9, 17, 26, 31, 40, 48, 55, 62, 69, 70, 77, 85, 93, 101, 110, 121, 129]
    multi = [7 * r + (k % 7) for k, r in enumerate(rows)]
    for k, s in enumerate(multi):
        lens[s] = (2, 4, 5, 9)[k % 4]
    seg_ptr = torch.zeros(7 * n + 1, dtype=torch.long)
    seg_ptr[1:] = torch.cumsum(lens, 0)
    g = torch.Generator().manual_seed(130)
    col = torch.zeros(int(seg_ptr[-1]), dtype=torch.long)
    for s in range(7 * n):
        lo, hi = (0, 70) if s // 7 < 70 else (70, 130)
        col[seg_ptr[s]:seg_ptr[s + 1]] = lo + torch.randperm(hi - lo, generator=g)[:int(lens[s])]
    return seg_ptr.to(torch.int32), col.to(torch.int32), torch.tensor(multi, dtype=torch.int32), bid, sizes


def counts(sizes):
    return torch.tensor([float(s) for s in sizes])


def apply_reference(x, bid, sizes, C, groups, w, b, act, count_eps, cS=0.0, cQ=0.0, eps=EPS, slack=0.0):
    """the whole chain on the host in float64 with its bound: (ref, S, c, (mean, rstd), sums) for sums carrying errors
    (cS, cQ) U of their magnitudes (0: exact sums -- the apply launches, which get the oracle's).  slack = 1 widens
    the mean by U |m| and rstd by U: the bound against a reference that divides by the count exactly
    (torch.nn.functional.group_norm) where the kernel multiplies by the fp32-rounded 1 / count."""
    B = len(sizes)
    s, mag = sums(x, bid, B)
    cnt = counts(sizes)
    mean, rstd = finalize(s[:, :, 0], s[:, :, 1], cnt, C, groups, eps, count_eps)
    dm, dr = stat_bounds(s[:, :, 0], s[:, :, 1], mag[:, :, 0], mag[:, :, 1], cS, cQ, U, cnt, C, groups, eps, count_eps)
    ref, S, _ = apply(x, bid, mean, rstd, w, b, act)
    dm, dr = dm + slack * U * mean.abs(), dr + slack * U
    return ref, S, apply_c(x, bid, mean, rstd, w, S, act, dm, dr), (mean, rstd), s
