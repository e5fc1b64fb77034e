"""float64 restatement of the kernels training starts and ends with -- csrc/ofx_loss.hip (ofx_octree_ce,
ofx_sdf_reg_loss, ofx_kl_sample_fwd / _bwd), ofx_gn_backward of csrc/ofx_norm.hip and csrc/ofx_points.hip (ofx_points_keys,
ofx_points_sort, ofx_octree_label_from_points, ofx_octree_point_features) -- written from include/ofx.h and the formulas
in the kernels' headers, with the bound constants the host tests (tests/test_train_oracle.py) and the device tests
(tests/test_gpu_loss_entry.py, test_gpu_gn_backward_entry.py, test_gpu_points_entry.py) share.  Nothing here imports
octfusion_amd; the comparison helper and the activations are glue_oracle's, the forward statistics gn_oracle's.

Every bounded comparison is glue_oracle.assert_close: |got - ref| <= c * 2^-24 * S elementwise, S = the sum of the
absolute values of the terms that form the element, c counted next to the formula.  Every function takes a `dtype`:
float64 is the reference, float32 an honest host evaluation of the same formula, which the host tests require to pass
the bounds the device tests use.  The counts use the project's figures for one fp32 operation in units of U = 2^-24
(glue_oracle): a sum or a product 1, expf within one ulp 2, a division within 2.5 ulp 5, sqrtf 1.
"""
import numpy as np
import torch

import glue_oracle as G
import gn_oracle as GN
from glue_oracle import U, assert_close          # noqa: F401

GRID_CAP = 8192 * 256          # threads of the largest launch (ofx_grid): work items past it take the grid-stride step
TINY = 2.0 ** -125             # S carries TINY so that c U S never falls below c steps (2^-149) of the subnormal range
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _np(dtype):
    return np.float32 if dtype in (np.float32, torch.float32, 'float32') else np.float64


# ------------------------------------------------------------------------------------------------ cross entropy
def ce_labels(child):
    """nempty_mask: label = child >= 0 (loss.py:117)"""
    return (np.asarray(child).astype(np.int64) >= 0).astype(np.int64)


def ce_hits(logits, child):
    """number of rows whose argmax equals the label; argmax returns the FIRST maximum: class 1 only where l1 > l0, so a
    tie -- -0.0 against 0.0 included, which compare equal -- is class 0"""
    l = np.asarray(logits, dtype=np.float32)
    return int(((l[:, 1] > l[:, 0]).astype(np.int64) == ce_labels(child)).sum())


def ce_margin(logits, child, dtype=np.float64):
    """d = l_other - l_label per row (exact in float64; one rounding in float32)"""
    l = np.asarray(logits, dtype=np.float32).astype(_np(dtype))
    lab = ce_labels(child)
    rows = np.arange(l.shape[0])
    return l[rows, 1 - lab] - l[rows, lab]


def ce_rows(logits, child, dtype=np.float64):
    """(ce, S) per row: the 2-class cross entropy as the softplus of d: ce = max(d, 0) + log1p(exp(-|d|)).  Both terms
    are non-negative: S = ce, nothing cancels -- m + log(e0 + e1) - l_label rounds a confident row's loss to 0."""
    d = ce_margin(logits, child, dtype)
    ce = np.maximum(d, 0) + np.log1p(np.exp(-np.abs(d)))
    return ce, ce.astype(np.float64)


def ce_rows_lse(logits, child):
    """the formulation ofx_octree_ce had before: fp32 m + log(e0 + e1) - l_label.  Kept for the host test that shows
    it misses the bound the softplus form keeps."""
    l = np.asarray(logits, dtype=np.float32)
    lab = ce_labels(child)
    m = np.maximum(l[:, 0], l[:, 1])
    lse = m + np.log(np.exp(l[:, 0] - m) + np.exp(l[:, 1] - m))
    return (lse - l[np.arange(l.shape[0]), lab]).astype(np.float32)


def ce_loss_bound(logits, child, ref_sum):
    """The bound of the summed loss: max(3 x the error of the float32 host evaluation on the same rows, n 2^-52 ref).
    The error of the host evaluation is taken row by row, sum_i max(|ce32_i - ce64_i|, U ce64_i): the quantity that
    bounds the error of the sum in ANY summation order.  (The signed error of one summation order is a random walk that
    may pass through 0 and bounds nothing; and a single row's fp32 value can be right by luck -- log1p(1) rounds to
    within 0.03 ulp of ln 2 -- where half an ulp of the row, U ce, is what any fp32 result may be off by.)  The second
    term is the fp64 summation of n non-negative terms.  Returns (bound, the host's sum of row errors, its signed sum
    error)."""
    ce64, _ = ce_rows(logits, child)
    ce32, _ = ce_rows(logits, child, np.float32)
    e = ce32.astype(np.float64) - ce64
    host = float(np.maximum(np.abs(e), U * ce64).sum())
    return max(3.0 * host, len(ce64) * 2.0 ** -52 * ref_sum), host, float(abs(e.sum()))


def ce_grad(logits, child, dscale, dtype=np.float64):
    """(dlogits [n, 2], S, c): s = sigmoid(d) of d = l_other - l_label goes as +s dscale to the other class and as
    -s dscale to the label -- (softmax - onehot) dscale without the cancellation of e inv - 1.  S = |the value| + TINY.
    c: d is rounded once and s answers a relative change of d with (1 - s) |d| (the only term that grows: 160 at the
    saturated rows); e = expf(-|d|) within one ulp (2), 1 + e (1), the division (5), e times it where d < 0 (1), dscale
    (1): c = 10 + |d| (1 - s)."""
    t = _np(dtype)
    d = ce_margin(logits, child, dtype)
    e = np.exp(-np.abs(d))
    s = np.where(d >= 0, t(1) / (t(1) + e), e / (t(1) + e))
    g = (s * t(np.float32(dscale))).astype(t)
    lab = ce_labels(child)
    out = np.empty((len(d), 2), dtype=t)
    rows = np.arange(len(d))
    out[rows, 1 - lab] = g
    out[rows, lab] = -g
    d64 = ce_margin(logits, child)
    e64 = np.exp(-np.abs(d64))
    one_minus_s = np.where(d64 >= 0, e64 / (1 + e64), 1 / (1 + e64))
    c = 10.0 + np.abs(d64) * one_minus_s
    return out, np.abs(out.astype(np.float64)) + TINY, np.repeat(c[:, None], 2, 1)


def ce_case_rows(kind, n, seed):
    """(logits [n, 2] float32, child [n]) of one kind of rows:
      'mix'     N(0, 3) logits with exact ties (0.5 / 0.5, -0.0 / 0.0, 0.0 / -0.0) and +-80 saturated rows, both ways
                round, in front; labels from a child holding -1, 0, INT32_MIN and INT32_MAX;
      (lo, hi)  correctly classified rows +-a, a uniform in the band: the split classifier late in training."""
    g = np.random.default_rng(seed)
    child = np.array([-1, 0, INT32_MIN, INT32_MAX], dtype=np.int64)[g.integers(0, 4, size=n)]
    if kind == 'mix':
        l = (g.standard_normal((n, 2)) * 3).astype(np.float32)
        # three ties under label 0 and two under label 1: counting a tie as class 1 changes the number of hits
        head = np.array([[0.5, 0.5], [-0.0, 0.0], [0.0, -0.0], [80.0, -80.0], [-80.0, 80.0], [0.5, 0.5], [-0.0, 0.0],
                         [1.0, 1.5], [80.0, -80.0], [-80.0, 80.0]], dtype=np.float32)[:n]
        l[:len(head)] = head
        child[:len(head)] = np.array([-1] * 5 + [0] * 5, dtype=np.int64)[:n]
        return l, child
    a = g.uniform(kind[0], kind[1], size=n).astype(np.float32)
    sign = np.where(child >= 0, 1.0, -1.0).astype(np.float32)          # label 1: l1 = +a
    return np.stack([-a * sign, a * sign], 1).astype(np.float32), child


CE_BANDS = [(0.0, 3.0), (4.0, 8.0), (8.0, 16.0)]


# ------------------------------------------------------------------------------------------------ sdf_reg
def sdf_reg(sdf, grad, sdf_gt, grad_gt, w_sdf, w_grad):
    """((sum (grad - grad_gt)^2, sum (sdf - sdf_gt)^2), dsdf, dgrad): the sums of the float64 squares of the fp32
    differences (every term exact and non-negative: any summation order is within terms 2^-53 relative);
    dsdf = cs e and dgrad = cg g as fp32 products with cs = 2 w_sdf / n and cg = 2 w_grad / (3 n) formed in fp32 as the
    host code forms them -- bit for bit."""
    f = np.float32
    n = len(sdf)
    e = np.asarray(sdf, f) - np.asarray(sdf_gt, f)
    gd = np.asarray(grad, f) - np.asarray(grad_gt, f)
    sums = (float((gd.astype(np.float64) ** 2).sum()), float((e.astype(np.float64) ** 2).sum()))
    if n == 0:
        return sums, e, gd
    cs = f(2.0) * f(w_sdf) / f(n)
    cg = f(2.0) * f(w_grad) / (f(3.0) * f(n))
    return sums, (cs * e).astype(f), (cg * gd).astype(f)


# ------------------------------------------------------------------------------------------------ posterior
LV_LO, LV_HI = -30.0, 20.0
KL_C_Z = 4.0          # expf (2), sd noise (1), the sum (1); an FMA saves one
KL_C_TERM = 6.0       # mean^2 (1), expf (2), three sums / differences (3) on partial sums of at most 2 S; 0.5 is exact
KL_C_DMEAN = 2.0      # kl_scale mean (1), the sum (1)
KL_C_DLV = 5.0        # g 0.5 sd noise: expf (2), two products (2); kl_scale 0.5 (var - 1): expf (2), var - 1 on var + 1
#                       (1), the product (1); the sum of the two (1) on top of the larger: 4 + 1


def posterior(params, noise, E, dtype=np.float64):
    """((z, S_z), (kl, S_kl)) elementwise [n, E]; params [n, >= 2E] = (mean | logvar): lv = clamp(logvar, -30, 20),
    z = mean + exp(lv / 2) noise (noise None: the mean), kl = 0.5 (mean^2 + var - 1 - lv) with
    S_kl = 0.5 (mean^2 + var + 1 + |lv|).  Near lv = 0 and mean = 0 the kl term cancels to far below S: that is the
    reference's own formula (distributions.py:46) and stays -- the bound is relative to S, not to the term."""
    t = _np(dtype)
    p = np.asarray(params, dtype=np.float32).astype(t)
    mean, lv = p[:, :E], np.clip(p[:, E:2 * E], t(LV_LO), t(LV_HI))
    sd, var = np.exp(t(0.5) * lv), np.exp(lv)
    nz = np.zeros_like(mean) if noise is None else np.asarray(noise, dtype=np.float32).astype(t)
    z = mean + sd * nz
    kl = t(0.5) * (mean * mean + var - t(1) - lv)
    m64, lv64, var64 = mean.astype(np.float64), lv.astype(np.float64), np.exp(lv.astype(np.float64))
    S_z = np.abs(m64) + np.abs(np.exp(0.5 * lv64) * nz.astype(np.float64))
    S_kl = 0.5 * (m64 * m64 + var64 + 1.0 + np.abs(lv64))
    return (z, S_z), (kl, S_kl)


def posterior_bwd(params, noise, dz, E, kl_scale, dtype=np.float64):
    """((dmean, S), (dlogvar, S)) of <dz, z> + kl_scale sum kl in closed form: dmean = dz + kl_scale mean;
    dlogvar = dz 0.5 sd noise + kl_scale 0.5 (var - 1) where the clamp passes, 0 where it blocks.  torch.clamp passes
    the gradient AT -30 and AT 20 and blocks it one ulp outside."""
    t = _np(dtype)
    p = np.asarray(params, dtype=np.float32).astype(t)
    mean, raw = p[:, :E], p[:, E:2 * E]
    lv = np.clip(raw, t(LV_LO), t(LV_HI))
    sd, var = np.exp(t(0.5) * lv), np.exp(lv)
    nz = np.zeros_like(mean) if noise is None else np.asarray(noise, dtype=np.float32).astype(t)
    g = np.zeros_like(mean) if dz is None else np.asarray(dz, dtype=np.float32).astype(t)
    ks = t(np.float32(kl_scale))
    dmean = g + ks * mean
    passes = (raw >= t(LV_LO)) & (raw <= t(LV_HI))
    t1, t2 = g * t(0.5) * sd * nz, ks * t(0.5) * (var - t(1))
    dlv = np.where(passes, t1 + t2, t(0))
    S_m = np.abs(g.astype(np.float64)) + np.abs(float(ks) * mean.astype(np.float64))
    S_l = np.where(passes, np.abs(t1.astype(np.float64)) + abs(float(ks)) * 0.5 * (np.exp(lv.astype(np.float64)) + 1.0), 0.0)
    return (dmean, S_m), (dlv, S_l)


def f32_next(v, toward):
    return float(np.nextafter(np.float32(v), np.float32(toward)))


def logvar_specials(hot=True):
    """exactly -30 and 20, one ulp inside and outside each, +-40 and 0; hot=False leaves out those that clamp to about
    20 (var = 4.9e8: four such terms carry U S = 30 each into the bound of the kl SUM, more than the few hundred terms
    the grid-stride step of the large cases adds, so those cases run without them)"""
    sp = np.array([-30.0, f32_next(-30, 0), f32_next(-30, -40), 20.0, f32_next(20, 0), f32_next(20, 40), -40.0, 40.0,
                   0.0], dtype=np.float32)
    return sp if hot else sp[np.array([0, 1, 2, 6, 8])]


def posterior_case(n, E, seed, hot=True):
    """(params [n, 2E], noise, dz): N(0, 1) with the special log-variances, four times over, in front"""
    g = np.random.default_rng(seed)
    params = g.standard_normal((n, 2 * E)).astype(np.float32)
    sp = logvar_specials(hot)
    k = min(n * E, 4 * len(sp))
    flat = params[:, E:].reshape(-1).copy()
    flat[:k] = np.tile(sp, 4)[:k]
    params[:, E:] = flat.reshape(n, E)
    return params, g.standard_normal((n, E)).astype(np.float32), g.standard_normal((n, E)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ GroupNorm backward
def gn_bwd_inputs(sizes, C, groups, seed):
    """(x, dy, bid): x as gn_oracle.make_x draws it but without its zero-variance group and its 1e-3 group -- the
    backward amplifies the fp32 rounding of the GIVEN mean by r^3 (conditioning 1 / (2 eps) on a constant group), a
    property of the operation --; dy ~ N(0, 1).  A group of a few values can land far from 0 on its own deviation by
    the draw: a group whose sample mean exceeds 6 sample deviations is shifted back to 6 (gn_conditioning then asserts
    |mean| <= 8 sigma with the operation's own mean and variance)."""
    g = torch.Generator().manual_seed(seed)
    B, n, cpg = len(sizes), sum(sizes), C // groups
    bid = GN.layout(sizes)
    i = bid.long()
    mu = torch.rand(B, groups, generator=g, dtype=torch.float64) * 4 - 2
    sd = torch.rand(B, groups, generator=g, dtype=torch.float64) * 3.75 + 0.25
    z = torch.randn(n, C, generator=g, dtype=torch.float64)
    x = mu[i].repeat_interleave(cpg, 1) + sd[i].repeat_interleave(cpg, 1) * z
    xg = x.reshape(n, groups, cpg)
    cnt = (torch.tensor(sizes, dtype=torch.float64) * cpg).clamp(min=1)[:, None]
    m = torch.zeros(B, groups, dtype=torch.float64).index_add_(0, i, xg.sum(2)) / cnt
    s = (torch.zeros(B, groups, dtype=torch.float64).index_add_(0, i, ((xg - m[i][:, :, None]) ** 2).sum(2)) / cnt).sqrt()
    shift = torch.where(m.abs() > 6 * s, m - torch.sign(m) * 6 * s, torch.zeros_like(m))
    shift = torch.where(s > 0, shift, torch.zeros_like(m))          # (a single value has no deviation to measure by)
    x = (xg - shift[i][:, :, None]).reshape(n, C)
    return x.float(), torch.randn(n, C, generator=g), bid


def gn_conditioning(x, bid, sizes, C, groups, eps=GN.EPS, count_eps=GN.EPS):
    """the largest |mean| / sigma over the non-empty (batch element, group)s, mean and sigma^2 = var as the operation
    defines them (count_eps included)"""
    m, _, var = gn_forward_stats(x.double(), bid, sizes, C, groups, eps, count_eps)
    full = torch.tensor(sizes) > 0
    return float((m.abs() / var.sqrt())[full].max()) if bool(full.any()) else 0.0


def gn_forward_stats(x, bid, sizes, C, groups, eps, count_eps):
    """differentiable float64 (m, r, var) [B, groups] of x exactly as gn_oracle.finalize states them: inv = 1 / (count
    cpg + count_eps) rounded to fp32, m = inv sum x, the centred variance inv sum (x - m)^2, r = (var + eps)^-1/2"""
    B, cpg = len(sizes), C // groups
    _, inv = GN._cnt_inv(GN.counts(sizes), cpg, count_eps)           # [B, 1] float64 of the fp32 value
    i = bid.long()
    xg = x.reshape(x.shape[0], groups, cpg)
    m = torch.zeros(B, groups, dtype=x.dtype).index_add_(0, i, xg.sum(2)) * inv.to(x.dtype)
    dev = xg - m[i][:, :, None]
    var = torch.zeros(B, groups, dtype=x.dtype).index_add_(0, i, (dev * dev).sum(2)) * inv.to(x.dtype)
    r = 1.0 / torch.sqrt(var + GN.f32(eps))
    return m, r, var


def gn_backward(x, dy, bid, sizes, C, groups, w, b, act, eps=GN.EPS, count_eps=GN.EPS, drop_count_eps_terms=False):
    """float64 autograd through y = act((x - m) r w + b), L = <dy, y>, with m and r functions of x (gn_forward_stats): the
    dependence on count_eps is in the graph, no coefficient formula is restated.  Returns a dict:
      dx, dgamma, dbeta      the gradients
      S_dx                   |w r g| + |c2 x| + |c3 - c2 mu|, g = dy act'(pre); c2 = 2 inv dL/dvar is read off the graph
                             (the gradient retained at var), the constant is what is left of dx
      S_dgamma, S_dbeta      sum over rows of |g (x - m) r| and of |g|
      m, r                   [B, C] float64 statistics
    drop_count_eps_terms=True treats sum (x - m) as 0 and the count as exact -- what a backward that ignored count_eps
    would compute; the host test shows it misses the bound where count_eps matters."""
    B, cpg = len(sizes), C // groups
    i = bid.long()
    with torch.enable_grad():
        xd = x.double().clone().requires_grad_(True)
        wd, bd = w.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)
        m, r, var = gn_forward_stats(xd, bid, sizes, C, groups, eps, 0.0 if drop_count_eps_terms else count_eps)
        var.retain_grad()
        mc, rc = m.repeat_interleave(cpg, 1), r.repeat_interleave(cpg, 1)
        pre = (xd - mc[i]) * rc[i] * wd + bd
        pre.retain_grad()
        y = G.act(pre, act)[0]
        (y * dy.double()).sum().backward()
    g = pre.grad
    _, inv = GN._cnt_inv(GN.counts(sizes), cpg, 0.0 if drop_count_eps_terms else count_eps)
    c2 = (2.0 * inv * var.grad).repeat_interleave(cpg, 1)[i]
    mcd, rcd = mc.detach(), rc.detach()
    lead = wd.detach() * rcd[i] * g
    const = xd.grad - lead - c2 * xd.detach()
    S_dx = lead.abs() + (c2 * xd.detach()).abs() + const.abs()
    S_dg = (g * (xd.detach() - mcd[i]) * rcd[i]).abs().sum(0)
    return dict(dx=xd.grad, dgamma=wd.grad, dbeta=bd.grad, S_dx=S_dx, S_dgamma=S_dg, S_dbeta=g.abs().sum(0), m=mcd, r=rcd,
                g=g, pre=pre.detach())


# the shapes of the device test: (C, groups) -- C / 4 = 9 and 24 do not divide 256, 1024 is the largest accepted width --
# and rows per batch element: ragged with an empty and a one-row element, and seventy one-row elements (more than two
# inside one 64-row block).  Where a group is ONE channel, one row is one value -- no variance, the conditioning the
# inputs exclude --, so those widths get two rows instead.
GN_WIDTHS = [(4, 1), (4, 4), (36, 1), (36, 36), (96, 1), (96, 96), (96, 32), (256, 1), (256, 256), (256, 32), (1024, 1),
             (1024, 1024), (1024, 32)]
GN_COUNT_EPS_WIDTHS = [(4, 1), (4, 4), (36, 9), (36, 36)]          # 4 and 1 channels per group
GN_COUNT_EPS_SIZES = (1, 2, 3, 1, 2, 3, 0, 2)


def gn_sizes(C, groups, rows):
    one = C // groups == 1
    if rows == 'ragged':
        return (200, 0, 63, 2 if one else 1, 64, 65)
    return ((2,) if one else (1,)) * 70


def gn_seed(C, groups, sizes):
    return C + groups + len(sizes)


def stats_rows(n, B, C=128):
    """rows per block of the statistics kernels (the rule stated at gn_stats_rows in ofx_norm.hip): 64, or a multiple
    of 64 once there are more 64-row chunks than blocks allowed -- 8 .. 128 per batch element by its bytes / 512 KB, at
    least 64 in all.  ofx_gn_backward asks with the default C = 128 whatever its C."""
    chunks = (n + 63) // 64
    per_batch = min(max(n * C * 4 // max(B, 1) // (512 << 10), 8), 128)
    cap = max(per_batch * B, 64)
    return 64 if chunks <= cap else 64 * ((chunks + cap - 1) // cap)


def act_grad(y, act):
    """act'(y) as the kernel writes it: silu s (1 + y (1 - s)), gelu 0.5 (1 + erf(y / sqrt 2)) + y phi(y)"""
    if act in (None, 'none'):
        return torch.ones_like(y)
    if act == 'silu':
        s = 1.0 / (1.0 + torch.exp(-y))
        return s * (1.0 + y * (1.0 - s))
    return 0.5 * (1.0 + torch.erf(y * 0.70710678118654752440)) + y * 0.3989422804014327 * torch.exp(-0.5 * y * y)


def _run_sums(v, bid, B, run):
    """[B, C] float64: per batch element, runs of `run` consecutive rows summed serially in fp32, the runs in float64"""
    out = torch.zeros(B, v.shape[1], dtype=torch.float64)
    for b in range(B):
        vb = v[bid == b]
        if vb.shape[0] == 0:
            continue
        vb = torch.cat([vb, torch.zeros(-vb.shape[0] % run, v.shape[1])]).view(-1, run, v.shape[1])
        a = torch.zeros(vb.shape[0], v.shape[1])
        for k in range(run):
            a = a + vb[:, k]
        out[b] = a.double().sum(0)
    return out


def gn_backward_f32(x, dy, bid, sizes, C, groups, w, b, act, eps=GN.EPS, count_eps=GN.EPS):
    """The float32 host evaluation of the same operation, by the scheme the header of the backward in ofx_norm.hip
    states: forward statistics as ofx_gn_stats + ofx_gn_finalize leave them (fp32 runs, fp64 across, mean and rstd
    rounded to fp32), g = dy act'(pre) in fp32, A = sum g and Bc = sum g x in fp32 runs of rows-per-block / rows-per-
    pass rows and fp64 across, the per-group coefficients in fp64 rounded to fp32, dx = k0 g + k1 x + k2 in fp32.
    Returns (dx, dgamma, dbeta) float32.  This is the floor an fp32 kernel of this design can reach; the bound of the
    device test is 3 x its worst ratio on the same inputs (gn_c)."""
    B, n, cpg = len(sizes), x.shape[0], C // groups
    i = bid.long()
    cnt = GN.counts(sizes)
    s, _ = GN.sums(x, bid, B, torch.float32, run=GN.stats_run(C, stats_rows(n, B, C)))
    mean, rstd = GN.finalize(s[:, :, 0], s[:, :, 1], cnt, C, groups, eps, count_eps, dtype=torch.float32)
    x, dy, w, b = x.float(), dy.float(), w.float(), b.float()
    g = dy * act_grad((x - mean[i]) * rstd[i] * w + b, act)
    run = -(-stats_rows(n, B) // (256 // (C // 4)))
    A, Bc = _run_sums(g, bid, B, run), _run_sums(g * x, bid, B, run)
    mu, r, wd = mean.double(), rstd.double(), w.double()
    grp = lambda t: t.reshape(B, groups, cpg).sum(2).repeat_interleave(cpg, 1)
    S1, S2 = grp(wd * A), grp(wd * (Bc - mu * A))
    _, inv = GN._cnt_inv(cnt, cpg, count_eps)
    ce = GN.f32(count_eps)
    c2 = 2.0 * inv * (-0.5 * r * r * r * S2)
    c3 = -inv * (r * S1 + c2 * mu * ce)
    k0, k1, k2 = (wd * r).float(), c2.float(), (c3 - c2 * mu).float()
    dx = k0[i] * g + k1[i] * x + k2[i]
    return dx, (r * (Bc - mu * A)).sum(0).float(), A.sum(0).float()


# the worst |host fp32 - ref| / (U S) of gn_backward_f32 over the shapes of the device test (GN_WIDTHS x both row layouts
# x the three activations), measured on the host: dx 1416 (C = 1024, one channel per group: a thread's fp32 run of 64 rows
# in the FORWARD statistics moves the mean by tens of U, which r^2 (x - mean) amplifies), dgamma 97, dbeta 98 (seventy
# two-row elements, one channel per group).  Recorded with headroom; tests/test_train_oracle.py recomputes them.
GN_HOST_RATIOS = (2000.0, 150.0, 150.0)
GN_C_FLOOR = 8.0         # the apply alone: three coefficients rounded to fp32 (3), g = dy act' (1), two products, two sums


def gn_c(ref, x, dy, bid, sizes, C, groups, w, b, act, eps=GN.EPS, count_eps=GN.EPS):
    """(c_dx, c_dgamma, c_dbeta, ratios): c = max(GN_C_FLOOR, 3 x the largest |host fp32 - ref| / (U S) of
    gn_backward_f32 on the same inputs).  The chain mean -> r^3 -> c2 amplifies the rounding of the given statistics by
    the conditioning of the group (|mean| / sigma, bounded by 8 in the test inputs), which no count of operations
    captures per element; the host evaluation measures it.  Worst host ratios over the cases of the device test, as
    tests/test_train_oracle.py recomputes them: see GN_HOST_RATIOS."""
    dx, dg, db = gn_backward_f32(x, dy, bid, sizes, C, groups, w, b, act, eps, count_eps)
    out, ratios = [], []
    for got, key in ((dx, 'dx'), (dg, 'dgamma'), (db, 'dbeta')):
        S = ref['S_' + key]
        ratio = float(((got.double() - ref[key]).abs() / (U * S.clamp(min=1e-300))).max()) if got.numel() else 0.0
        ratios.append(ratio)
        out.append(max(GN_C_FLOOR, 3.0 * ratio))
    return out[0], out[1], out[2], ratios


# ------------------------------------------------------------------------------------------------ points
def spread3(v):
    v = np.asarray(v, dtype=np.uint64)
    out = np.zeros_like(v)
    for i in range(16):
        out |= ((v >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i)
    return out


def morton(x, y, z):
    """level-bit i of x -> key bit 3i + 2, y -> 3i + 1, z -> 3i"""
    return ((spread3(x) << np.uint64(2)) | (spread3(y) << np.uint64(1)) | spread3(z)).astype(np.int64)


def scaled(pts, depth):
    """fp32 (p + 1) * 2^(depth-1): two roundings, the second exact (a power of two)"""
    return (np.asarray(pts, np.float32)[:, :3] + np.float32(1)) * np.float32(2 ** (depth - 1))


def points_keys(pts, batch, depth):
    """batch << 48 | morton(clamp(trunc(fp32 (p + 1) 2^(depth-1)), 0, 2^depth - 1)); batch an array or one number"""
    q = np.clip(np.trunc(scaled(pts, depth)).astype(np.int64), 0, 2 ** depth - 1)
    b = np.broadcast_to(np.asarray(batch, dtype=np.int64), (len(q),))
    return (b << 48) | morton(q[:, 0], q[:, 1], q[:, 2])


def points_sort(keys, idx):
    """a stable sort of the (key, idx) pairs by key: equal keys keep their input order"""
    perm = np.argsort(np.asarray(keys, dtype=np.int64), kind='stable')
    return np.asarray(keys)[perm], np.asarray(idx)[perm]


def label_from_points(sorted_keys, node_keys, depth_pts, d):
    """label[j] = 1 iff the sorted finest-depth keys hold one inside the cell of node j of depth d: the cell is the
    half-open key range [lo, lo + 8^(depth_pts - d)), lo = batch << 48 | morton_d << 3 (depth_pts - d)"""
    k = np.asarray(node_keys, dtype=np.int64)
    shift = 3 * (depth_pts - d)
    lo = ((k >> 48) << 48) + ((k & ((1 << 48) - 1)) << shift)
    sk = np.asarray(sorted_keys, dtype=np.int64)
    return (np.searchsorted(sk, lo, 'left') < np.searchsorted(sk, lo + (1 << shift), 'left')).astype(np.int64)


# avg_points: the sums are exact by construction of the test's inputs, the division is one rounding: 2 U covers 2.5 ulp
# less -- the bound the issue of this suite sets
POINTS_C_AVG = 2.0
# the normal: three squares and two sums of non-negative terms move len^2 by 3 U, the root halves that (1.5) and rounds
# (1), the reciprocal (5), the product (1)
POINTS_C_NORMAL = 8.5
# the dot product against S = sum_k (|a_k| + |trunc a_k| + 0.5) |n_k|: the rounded average (POINTS_C_AVG; a - trunc a is
# exact), - 0.5 (1), the normal's own error, three products (1 on each term), two sums (2)
POINTS_C_DOT = POINTS_C_AVG + 1.0 + POINTS_C_NORMAL + 1.0 + 2.0


def point_features(sorted_keys, sorted_idx, pts, normals, node_keys, depth, dtype=np.float64):
    """(feat [nnum, 4], avg_points [nnum, 3], avg_normals [nnum, 3], S_dot [nnum], exact): per node of the finest depth,
    over the points whose key equals the node's in sorted (= input) order: the serial sums of the fp32 scaled positions
    and of the normals, avg = sum / count, normal = sum / max(|sum|, 1e-12), feat = (normal, dot(frac(avg) - 0.5,
    normal)); zero rows for empty nodes.  `exact` is True iff every fp32 partial sum equalled the float64 one."""
    t = _np(dtype)
    sk, si = np.asarray(sorted_keys, dtype=np.int64), np.asarray(sorted_idx, dtype=np.int64)
    q = scaled(pts, depth) if len(si) else np.zeros((0, 3), np.float32)
    nk = np.asarray(node_keys, dtype=np.int64)
    lo, hi = np.searchsorted(sk, nk, 'left'), np.searchsorted(sk, nk, 'right')
    nnum = len(nk)
    feat, avg, nrm, S = np.zeros((nnum, 4), t), np.zeros((nnum, 3), t), np.zeros((nnum, 3), t), np.zeros(nnum)
    exact = True
    for j in np.nonzero(hi > lo)[0]:
        rows = si[lo[j]:hi[j]]
        sp, sn = np.zeros(3, t), np.zeros(3, t)
        sp32, sn32 = np.zeros(3, np.float32), np.zeros(3, np.float32)
        for r in rows:
            sp = sp + q[r].astype(t)
            sp32 = sp32 + q[r]
            if normals is not None:
                sn = sn + np.asarray(normals[r, :3], np.float32).astype(t)
                sn32 = sn32 + np.asarray(normals[r, :3], np.float32)
            exact = exact and bool(np.all(sp32.astype(np.float64) == sp.astype(np.float64))) and \
                bool(np.all(sn32.astype(np.float64) == sn.astype(np.float64)))
        a = sp / t(len(rows))
        length = np.sqrt((sn * sn).sum(dtype=t))
        v = sn * (t(1) / np.maximum(length, t(np.float32(1e-12))))
        local = a - np.trunc(a) - t(0.5)
        avg[j], nrm[j] = a, v
        feat[j, :3], feat[j, 3] = v, (local * v).sum(dtype=t)
        S[j] = float(((np.abs(a) + np.abs(np.trunc(a)) + 0.5) * np.abs(v)).astype(np.float64).sum())
    return feat, avg, nrm, S, exact
