"""Host-side oracle for the attention entry points (csrc/ofx_dense.hip: ofx_attention, ofx_attention_bwd): QKVAttention
restated in float64 with an elementwise worst-case fp32 bound, its float64 autograd, seeded input makers that put the
softmax where a kernel goes wrong, and a mirror of the launcher's arithmetic that names the route a case takes.  No GPU, no
octfusion_amd.  tests/test_attention_oracle.py shows that the bound accepts honest fp32 arithmetic with room and rejects
planted errors; tests/test_gpu_attention_entry.py holds the kernels to it.

Row layout: qkv [B * T, 3 * heads * ch], channel = head * 3 * ch + {q: 0..ch | k: ch..2ch | v: 2ch..3ch}; out [B * T, heads * ch],
channel = head * ch + c.  scale = ch ** -0.25 on q and on k.

The bound (u = 2^-24, the unit roundoff of fp32; first order in u; the constants count roundings, none is fitted):

  scores.  s_ij = sum_c (q_ic scale)(k_jc scale) in fp32: each product carries the two scalings and its own rounding (3 u),
  and a sum of ch terms in any order adds at most ch - 1 roundings to a term, so
      |s~_ij - s_ij| <= (ch + 2) u a_ij,   a_ij = sum_c |q_ic k_jc| scale^2,
  and Delta_i = (ch + 4) u max_j a_ij holds for every key of query i with two roundings to spare (the scale itself is
  a constant with a few roundings of its own: they move every score by the same relative amount).

  softmax.  With x_ij = s_ij - max_j s_ij and p_ij = exp(x_ij) / sum_j exp(x_ij): scores off by at most Delta_i each move
  the numerator by a factor within exp(+-Delta_i) and the denominator, a positive combination, likewise: 2 Delta_i relative
  on p_ij.  The fast exp is exp2(x log2 e): the subtraction that makes x rounds once (|x| u absolute in the argument,
  |x| u relative in the result), the product with log2 e once more (again |x| u), and the hardware exp2 is good to 1 ulp
  (2 u); with two to spare that is (4 + 2 |x_ij|) u on every exponential, and the same on the denominator's: the factor
  2.  The denominator is a sum of T positive terms in an order the oracle does not know, then 1 / sum and the product
  with it; the output is again a sum over T keys whose roundings are relative to partial sums of mixed sign, bounded through
  sum_j p_ij |v_jc|: (T + 4) u covers the T - 1 additions of whichever of the two is longer plus the division, the
  product and the MFMA's product rounding.  Together
      rel_ij   = 2 Delta_i + 2 (4 + 2 |x_ij|) u + (T + 4) u
      bound_ic = sum_j p_ij rel_ij |v_jc|.
  The output's own T - 1 additions are the one place where this is generous rather than strict (they add to the T + 4
  instead of being counted on top of the denominator's); fp32 on the CPU uses 0.06 of the bound at worst."""
import collections
import math

import torch

U = 2.0 ** -24

KINDS = ('plain', 'peaked', 'offset', 'negative', 'lastkey')

# (B, T, heads, ch): the smallest shape that reaches each path of attention_mfma_kernel (see path())
FWD_SHAPES = [(2, 1, 2, 6), (3, 33, 2, 30), (2, 100, 3, 40), (1, 97, 1, 100), (1, 127, 2, 65), (2, 128, 2, 128), (2, 255, 4, 16),
              (2, 257, 2, 24), (1, 287, 1, 64), (1, 530, 2, 32)]
LAYOUT_SHAPES = [(3, 33, 2, 32), (2, 100, 3, 40), (2, 257, 2, 24)]
BWD_SHAPES = [(2, 1, 2, 6), (3, 33, 2, 30), (2, 100, 3, 40), (1, 97, 1, 100), (1, 65, 2, 128), (2, 257, 2, 24), (1, 511, 1, 12),
              (1, 512, 1, 8)]
BWD_KINDS = ('plain', 'peaked', 'lastkey')


def fwd_kinds(T):
    """Every shape runs plain and negative; the ones with more than one key tile also peaked, offset and lastkey."""
    return ('plain', 'negative') + (('peaked', 'offset', 'lastkey') if T > 32 else ())


def fwd_cases():
    """Every (shape, input kind) the GPU file puts through the forward kernel, the layout shapes (plain) included."""
    return [(s, k) for s in FWD_SHAPES for k in fwd_kinds(s[1])] + [(s, 'plain') for s in LAYOUT_SHAPES]


def seed_of(shape, kind):
    B, T, heads, ch = shape
    return ((B * 1000 + T) * 10 + heads) * 1000 + ch * 7 + KINDS.index(kind)


def make(kind, B, T, heads, ch, seed=None):
    """Seeded qkv [B * T, 3 * heads * ch] in float32.  e = ones / sqrt(ch), so an offset a ch^0.25 e on q and b ch^0.25 e
    on k adds a * b to every score."""
    g = torch.Generator().manual_seed(seed_of((B, T, heads, ch), kind) if seed is None else seed)
    x = torch.randn(B, T, heads, 3, ch, generator=g, dtype=torch.float64) * (6.0 if kind == 'peaked' else 1.5)
    e = ch ** 0.25 / math.sqrt(ch)
    if kind == 'offset':            # every score near +100, close together: the max subtraction
        x[:, :, :, 0] += 10 * e
        x[:, :, :, 1] += 10 * e
    elif kind == 'negative':        # every real score near -36: a padded key let in at score 0 takes the softmax
        x[:, :, :, 0] += 6 * e
        x[:, :, :, 1] -= 6 * e
    elif kind == 'lastkey':         # every query attends key T - 1: a mask off by one changes every output element
        x[:, :, :, 0] += 4 * e
        x[:, T - 1, :, 1] += 8 * e
    elif kind not in ('plain', 'peaked'):
        raise ValueError(kind)
    return x.reshape(B * T, 3 * heads * ch).float()


def _qkv(qkv, B, T, heads, dtype):
    C = qkv.shape[1] // 3
    ch = C // heads
    assert qkv.shape == (B * T, 3 * heads * ch), (qkv.shape, B, T, heads)
    x = qkv.to(dtype).view(B, T, heads, 3, ch)
    return x[:, :, :, 0], x[:, :, :, 1], x[:, :, :, 2], ch                     # [B, T, heads, ch]


def evaluate(qkv, B, T, heads, dtype=torch.float64):
    """QKVAttention in `dtype` (differentiable): out [B * T, heads * ch]."""
    q, k, v, ch = _qkv(qkv, B, T, heads, dtype)
    scale = ch ** -0.25
    p = torch.softmax(torch.einsum('bthc,bshc->bhts', q * scale, k * scale), dim=-1)
    return torch.einsum('bhts,bshc->bthc', p, v).reshape(B * T, heads * ch)


def forward(qkv, B, T, heads):
    """(out64, bound): the float64 result and the elementwise fp32 bound derived in the module docstring."""
    q, k, v, ch = _qkv(qkv, B, T, heads, torch.float64)
    scale = ch ** -0.25
    s = torch.einsum('bthc,bshc->bhts', q * scale, k * scale)
    a = torch.einsum('bthc,bshc->bhts', q.abs(), k.abs()) * (scale * scale)
    delta = (ch + 4) * U * a.max(dim=-1, keepdim=True).values
    x = s - s.max(dim=-1, keepdim=True).values
    p = torch.softmax(s, dim=-1)
    rel = 2 * delta + 2 * (4 + 2 * x.abs()) * U + (T + 4) * U
    out = torch.einsum('bhts,bshc->bthc', p, v).reshape(B * T, heads * ch)
    bound = torch.einsum('bhts,bshc->bthc', p * rel, v.abs()).reshape(B * T, heads * ch)
    return out, bound


def values(qkv, B, T, heads):
    """The v block of every head in the layout of the output (what attention over a single key returns)."""
    return _qkv(qkv, B, T, heads, qkv.dtype)[2].reshape(B * T, -1)


def backward(qkv, dout, B, T, heads):
    """(dqkv64, dqkv32): autograd of the float64 forward, and the same formula in float32 on the CPU -- the latter
    against the former is the noise floor an fp32 kernel is judged by."""
    def grad(dtype):
        with torch.enable_grad():
            x = qkv.to(dtype).requires_grad_(True)
            (evaluate(x, B, T, heads, dtype) * dout.to(dtype)).sum().backward()
        return x.grad
    return grad(torch.float64), grad(torch.float32)


def ratio(got, ref, bound):
    """Worst |got - ref| / bound; an element with bound 0 must be exact."""
    d = (got.double() - ref).abs()
    if bool(((bound == 0) & (d > 0)).any()):
        return float('inf')
    return float((d / bound.clamp(min=1e-300)).max())


# ------------------------------------------------------------------------------------------------ the launcher's arithmetic
Path = collections.namedtuple('Path', 'width split staging accepted')
LDS_LIMIT = 160 * 1024 - 2048


def path(T, ch, ldq, ld_other=None, aligned=True, split_on=True):
    """The route of a launch.  width: the template's head width; split: the split-keys kernel; staging: 'float4' or the
    reason for the scalar loop ('ch', 'pitch', 'base': the first that applies, in the order the kernel tests them);
    accepted: the LDS rule 2 * Tp * (width + 4) * 4 <= 160 KiB - 2 KiB.  ld_other is the pitch of dout for the backward
    kernels (their branch wants it a multiple of 4 as well; width, split and accepted describe the forward), `aligned`
    says that every operand the branch looks at starts on a 16-byte boundary."""
    assert 1 <= ch <= 128
    width = 32 if ch <= 32 else (64 if ch <= 64 else 128)
    Tp = (T + 31) // 32 * 32
    if ch % 4:
        staging = 'ch'
    elif ldq % 4 or (ld_other is not None and ld_other % 4):
        staging = 'pitch'
    elif not aligned:
        staging = 'base'
    else:
        staging = 'float4'
    return Path(width, bool(T >= 256 and split_on), staging, 2 * Tp * (width + 4) * 4 <= LDS_LIMIT)


def split_tiles(T):
    """Key tiles of the four waves of the split-keys kernel: wave w takes tiles [w n / 4, (w + 1) n / 4)."""
    n = (T + 31) // 32
    return [(w + 1) * n // 4 - w * n // 4 for w in range(4)]
