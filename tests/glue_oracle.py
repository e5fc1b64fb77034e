"""float64 torch restatement of the glue operators (csrc/ofx_misc.hip and ofx_act through octfusion_amd.ops), written
from the formulas of include/ofx.h ("glue ops") and the reference lines cited there, plus the one comparison helper
the tests of these operators share.  Nothing here imports octfusion_amd.

Every reference returns (ref, S): the float64 result and, per element, the MAGNITUDE S = the sum of the absolute values
of the terms that form the element.  `assert_close` asserts |got - ref| <= c * 2^-24 * S elementwise: the bound of one
element does not depend on any other, so a wrong small output cannot hide behind a large one, and a term that was
dropped, or taken from a neighbour, is off by about S / (number of terms) -- many orders above c * 2^-24 * S.

All functions take a `dtype` (default float64).  With dtype=torch.float32 they are an honest fp32 evaluation of the
same formula on the host: tests/test_glue_oracle.py requires those to pass the bounds the GPU tests use.
"""
import math

import torch

U = 2.0 ** -24          # unit roundoff of fp32: one correctly rounded operation has a relative error <= U
F32_CLAMP = float(torch.tensor(1e-8, dtype=torch.float32))          # the kernel's 1e-8f

ACTS = (None, 'silu', 'gelu')
# max |act'(v)|: an error e in the argument becomes at most L * e in the result
LIPSCHITZ = {None: 1.0, 'silu': 1.0999, 'gelu': 1.1290}


def act(x, kind):
    """(act(x), S).  silu = x * sigmoid(x) has one term.  gelu = 0.5 x + 0.5 x erf(x / sqrt 2) has two, which cancel
    for x < 0: S = 0.5 |x| (1 + |erf|) is |gelu(x)| for x >= 0 and larger for x < 0 -- the conditioning of the formula
    (torch.nn.functional.gelu evaluates the same one), which no fp32 evaluation of it can beat."""
    if kind in (None, 'none'):
        return x.clone(), x.abs()
    if kind == 'silu':
        y = x * torch.sigmoid(x)
        return y, y.abs()
    assert kind == 'gelu'
    e = torch.erf(x * (1.0 / math.sqrt(2.0)))
    return 0.5 * x * (1.0 + e), 0.5 * x.abs() * (1.0 + e.abs())


def act_c(x, kind):
    """Error of ONE fp32 evaluation of act(x), as a factor c (elementwise) of U * S with S from act():
      silu: v / (1 + exp(-v)) with the exponential as exp2(-v * log2 e): the product and the rounded constant move the
            exponent by 2 |v| U relative (2 |v|), the hardware exp2 is within one ulp (2), both scaled by the
            sensitivity exp(-v) / (1 + exp(-v)) = sigmoid(-v) <= 1 of the quotient to it; the sum (1) and a division
            within 2.5 ulp (5): c = 10 + 2 |v| sigmoid(-v)  (|v| sigmoid(-v) <= 0.28 for v >= 0: five ulp there)
      gelu: erf within 4 ulp (8 |erf|), its rounded argument (2 x erf'(x) |x| <= 1), the sum (1 + |erf|), two
            products (2): c = 12."""
    if kind in (None, 'none'):
        return torch.zeros_like(x, dtype=torch.float64)
    if kind == 'silu':
        xd = x.double()
        return 10.0 + 2.0 * xd.abs() * torch.sigmoid(-xd)
    return torch.full_like(x, 12.0, dtype=torch.float64)


def linear_small(a, w, bias=None, res=None, act_in=None, act_out=None, dtype=torch.float64):
    """out = act_out(act_in(a) @ w^T + bias + res), w [N, K] (ofx.h: ofx_linear_small).
    Returns (ref, S, pre): S = sum_k S_in(a)_k |w_k| + |bias| + |res| and pre = the value act_out is applied to."""
    a, w = a.to(dtype), w.to(dtype)
    x, xs = act(a, act_in)
    pre = x @ w.t()
    S = xs.double() @ w.double().abs().t()
    if bias is not None:
        pre = pre + bias.to(dtype)
        S = S + bias.double().abs()
    if res is not None:
        pre = pre + res.to(dtype)
        S = S + res.double().abs()
    return act(pre, act_out)[0], S, pre


def linear_small_c(a, K, bias, res, act_in, act_out):
    """c of ofx_linear_small's bound, from the kernel's summation: a lane adds its share of K serially with one
    rounding per FMA -- 4 per 256 columns in the float4 loop, 1 per 64 in the scalar loop; the larger of the two
    covers either --, six xor-shuffle levels add the 64 lanes, the epilogue adds bias and res (one rounding each); the
    error of act_in's own evaluation (act_c, its largest value over the operand) enters like one more rounding of every
    term.  A sum of depth D is within D U sum |terms|.  act_out turns that error into at most L times as much and adds
    its own evaluation error c_out U S_out(v) with S_out(v) <= |v| <= S: silu 10 + 2 |v| sigmoid(-v) sigmoid(v) <= 10.5,
    gelu 12."""
    steps = max(4 * ((K + 255) // 256), (K + 63) // 64)
    c_in = float(act_c(a, act_in).max()) if a.numel() else 0.0
    depth = c_in + steps + 6 + (bias is not None) + (res is not None)
    c_out = {None: 0.0, 'silu': 10.5, 'gelu': 12.0}[act_out]
    return depth * LIPSCHITZ[act_out] + c_out


def rows_copy(src, dst, n, smap=None, dmap=None, C=None):
    """dst[dmap(i), 0:C] = src[smap(i), 0:C] for i < n; a negative entry of either map skips i.  Returns the new dst
    (a copy) and the bool mask of the destination rows that were written."""
    C = src.shape[1] if C is None else C
    out = dst.clone()
    hit = torch.zeros(dst.shape[0], dtype=torch.bool)
    idx = torch.arange(n)
    sr = smap[:n].long() if smap is not None else idx
    dr = dmap[:n].long() if dmap is not None else idx
    ok = (sr >= 0) & (dr >= 0)
    out[dr[ok], :C] = src[sr[ok], :C]
    hit[dr[ok]] = True
    return out, hit


def timestep_embedding(t, dim, max_period=10000.0, dtype=torch.float64):
    """[cos(t f) | sin(t f) | 0 if dim is odd], f_k = exp(-ln(max_period) k / half), half = dim // 2
    (ldm_diffusion_util.py:171-191)."""
    half = dim // 2
    f = torch.exp(-math.log(max_period) * torch.arange(half, dtype=dtype) / half)
    arg = t.to(dtype)[:, None] * f[None]
    out = torch.cat([torch.cos(arg), torch.sin(arg)], dim=1)
    if dim % 2:
        out = torch.cat([out, torch.zeros_like(out[:, :1])], dim=1)
    return out


def learned_sinusoid(t, w, dtype=torch.float64):
    """[t | sin(2 pi t w) | cos(2 pi t w)], the argument formed as ((t w) 2) pi (modules.py:550-563)."""
    t, w = t.to(dtype), w.to(dtype)
    arg = t[:, None] * w[None, :] * 2 * math.pi
    return torch.cat([t[:, None], torch.sin(arg), torch.cos(arg)], dim=1)


def ddim_eps(x, eps, coef, dtype=torch.float64, clamp=True):
    """coef = (alpha, sigma, alpha_next, sigma_next): x0 = (x - eps sigma) / max(alpha, 1e-8);
    x' = x0 alpha_next + eps sigma_next (octfusion_model_union.py:345-350).  Returns (x', S', x0, S0)."""
    x, eps = x.to(dtype), eps.to(dtype)
    alpha, sigma, alpha_n, sigma_n = [coef[i].to(dtype) for i in range(4)]
    a = torch.clamp(alpha, min=F32_CLAMP) if clamp else alpha
    x0 = (x - eps * sigma) / a
    S0 = (x.double().abs() + (eps.double() * sigma.double()).abs()) / a.double()
    xn = x0 * alpha_n + eps * sigma_n
    Sn = S0 * alpha_n.double().abs() + (eps.double() * sigma_n.double()).abs()
    return xn, Sn, x0, S0


# roundings on the way to x0: the product, the difference (2 U (|x| + |eps sigma|) together), a division within 2.5 ulp
# (5), the clamp constant 1e-8f against 1e-8 (1) -- and from there to x': two products and the sum, each on at most S'
DDIM_EPS_C_X0 = 8.0
DDIM_EPS_C_X = DDIM_EPS_C_X0 + 3.0


def ddim_x0(x, x0, noise, coef, dtype=torch.float64):
    """coef = (alpha, c, alpha_next, sd): x' = alpha_next (x (1 - c) / alpha + c x0) + sd noise (:326-344).
    Returns (x', S)."""
    x, x0 = x.to(dtype), x0.to(dtype)
    alpha, c, alpha_n, sd = [coef[i].to(dtype) for i in range(4)]
    mean = alpha_n * (x * (1.0 - c) / alpha + c * x0)
    S = alpha_n.double().abs() * ((x.double() * (1.0 - c.double()) / alpha.double()).abs() + (c.double() * x0.double()).abs())
    out = mean
    if noise is not None:
        out = mean + sd * noise.to(dtype)
        S = S + (sd.double() * noise.double()).abs()
    return out, S


# the longest chain: 1 - c (1), x (1 - c) (1), the division within 2.5 ulp (5), the inner sum (1), alpha_next (1), the
# outer sum (1); c x0 and sd noise are shorter
DDIM_X0_C = 10.0


def group_sums(x, batch_id, B):
    """fp64 [B, C, 2]: (sum x, sum x^2) per batch element and channel -- the statistics a producer attaches."""
    C = x.shape[1]
    s = torch.zeros(B, C, 2, dtype=torch.float64)
    s[:, :, 0].index_add_(0, batch_id.long(), x.double())
    s[:, :, 1].index_add_(0, batch_id.long(), x.double() ** 2)
    return s


def assert_close(got, ref, S, c, what=''):
    """|got - ref| <= c * 2^-24 * S for every element (c a number or a tensor); NaN or inf in `got` fails."""
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    S = torch.as_tensor(S).detach().cpu().double().expand_as(ref)
    bound = torch.as_tensor(c, dtype=torch.float64).cpu() * U * S
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    bad = ~(err <= bound)                 # (NaN compares false: it is bad)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError('%s: %d of %d elements off; first flat index %d: got %r ref %r |err| %.3e bound %.3e' % (
            what, int(bad.sum()), bad.numel(), i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]),
            float(err.reshape(-1)[i]), float(bound.expand_as(err).reshape(-1)[i])))
    used = err / bound.clamp(min=1e-300)
    return float(used[bound.expand_as(err) > 0].max()) if bool((bound > 0).any()) else 0.0
