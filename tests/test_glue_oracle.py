"""tests/glue_oracle.py against itself, on the host: every bound the GPU tests of the glue operators use
(tests/test_gpu_glue.py) must ACCEPT an honest float32 evaluation of the same formula and must REJECT a set of planted
errors of the kind a subtly wrong kernel makes -- a dropped k term, a column taken from its neighbour, a row taken from
row M - 1 (the clamp leaking), sin / cos halves swapped, a non-zero trailing column, a skipped row written, the alpha
clamp missing.  So a green GPU run means something, and the bounds leave room for fp32 arithmetic."""
import math

import pytest
import torch

import glue_oracle as G

torch.set_grad_enabled(False)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _linear_case(M, K, N, act_in, act_out, seed=0):
    g = _gen(seed)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    return a, w, bias, res


@pytest.mark.parametrize('act_in', G.ACTS)
@pytest.mark.parametrize('act_out', G.ACTS)
@pytest.mark.parametrize('M,K,N', [(1, 4, 1), (3, 17, 3), (5, 260, 17), (16, 1028, 30)])
def test_float32_linear_passes(M, K, N, act_in, act_out):
    a, w, bias, res = _linear_case(M, K, N, act_in, act_out)
    ref, S, _ = G.linear_small(a, w, bias, res, act_in, act_out)
    got = G.linear_small(a, w, bias, res, act_in, act_out, dtype=torch.float32)[0]
    G.assert_close(got, ref, S, G.linear_small_c(a, K, bias, res, act_in, act_out), 'float32 linear')


@pytest.mark.parametrize('plant', ['dropped_k', 'neighbour_column', 'clamped_row'])
@pytest.mark.parametrize('act_in,act_out', [(None, None), ('silu', 'gelu'), ('gelu', 'silu')])
@pytest.mark.parametrize('M,K,N', [(3, 17, 3), (9, 1028, 30)])
def test_planted_linear_errors_fail(M, K, N, act_in, act_out, plant):
    a, w, bias, res = _linear_case(M, K, N, act_in, act_out, seed=1)
    ref, S, _ = G.linear_small(a, w, bias, res, act_in, act_out)
    c = G.linear_small_c(a, K, bias, res, act_in, act_out)
    if plant == 'dropped_k':
        w2 = w.clone()
        w2[N - 1, K - 1] = 0.0                                    # one term of one column
        got = G.linear_small(a, w2, bias, res, act_in, act_out)[0]
    elif plant == 'neighbour_column':
        got = ref.clone()
        pre = G.linear_small(a, w, None, None, act_in, None)[0]
        pre[:, N - 1] = pre[:, N - 2]                             # weight row N - 2 used for column N - 1
        got[:, N - 1] = G.act(pre + bias.double() + res.double(), act_out)[0][:, N - 1]
    else:
        a2 = a.clone()
        a2[M - 2] = a[M - 1]                                      # row M - 2 read from row M - 1
        got = G.linear_small(a2, w, bias, res, act_in, act_out)[0]
    G.assert_close(ref.float(), ref, S, c, 'the rounded reference itself')
    with pytest.raises(AssertionError):
        G.assert_close(got.float(), ref, S, c, plant)


@pytest.mark.parametrize('kind', G.ACTS)
def test_float32_act_passes_and_a_wrong_one_fails(kind):
    x = torch.cat([torch.tensor([0.0, -0.0, 100.0, -100.0, 1e4, -1e4]), torch.linspace(-8, 8, 1001),
                   torch.randn(1000, generator=_gen(2)) * 3])
    ref, S = G.act(x.double(), kind)
    got = G.act(x, kind)[0]
    assert got.dtype == torch.float32
    big = ref.abs() > 2.0 ** -100
    c = G.act_c(x, kind).clamp(min=1.0)
    G.assert_close(got[big], ref[big], S[big], c[big], 'float32 ' + str(kind))
    wrong = got * (1 + 2.0 ** -17)                                 # 64 ulp
    nz = big & (S <= ref.abs() * 1.0001)                           # where S is the value itself: a relative bound
    assert bool(nz.any())
    with pytest.raises(AssertionError):
        G.assert_close(wrong[nz], ref[nz], S[nz], c[nz], 'scaled')
    if kind is not None:
        other = G.act(x, 'gelu' if kind == 'silu' else 'silu')[0]
        with pytest.raises(AssertionError):
            G.assert_close(other[big], ref[big], S[big], c[big], 'the other activation')


def _emb_margin(f32, f64, t):
    """the GPU tests' bound: per value of t, four times the largest float32-vs-float64 difference of the reference"""
    out = {}
    for v in sorted(set(t.tolist())):
        rows = t == v
        out[v] = 4.0 * float((f32[rows].double() - f64[rows]).abs().max())
    return out


@pytest.mark.parametrize('dim', [2, 3, 17, 64, 513])
def test_timestep_embedding_layout_and_planted_errors(dim):
    t = torch.tensor([0.0, 1.0, 0.5, 37.25, 999.0])
    half = dim // 2
    ref = G.timestep_embedding(t, dim, 10000.0)
    f32 = G.timestep_embedding(t, dim, 10000.0, dtype=torch.float32)
    assert ref.shape == (5, dim) and f32.dtype == torch.float32
    # the same function as the oracle's, which the end-to-end goldens use
    from oracle import unet as OU
    assert torch.equal(f32, OU.timestep_embedding(t, dim, 10000))
    assert torch.allclose(ref[:, :half], torch.cos(t.double()[:, None] * torch.exp(
        -math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)))
    if dim % 2:
        assert bool((ref[:, -1] == 0).all()) and bool((f32[:, -1] == 0).all())
    margin = _emb_margin(f32, ref, t)
    assert margin[0.0] == 0.0 and margin[1.0] <= 1e-6              # no amplification at t in {0, 1}

    def ok(got):
        return all(float((got[i].double() - ref[i]).abs().max()) <= margin[float(t[i])] for i in range(len(t)))
    assert ok(f32)
    swapped = torch.cat([f32[:, half:2 * half], f32[:, :half], f32[:, 2 * half:]], dim=1)
    assert not ok(swapped)
    if dim % 2:
        dirty = f32.clone()
        dirty[:, -1] = 1e-30
        assert not bool((dirty[:, -1] == 0).all())
    if half > 1:
        shifted = f32.clone()
        shifted[:, 1] = f32[:, 0]                                   # a column from its neighbour
        assert not ok(shifted)


@pytest.mark.parametrize('half', [1, 8, 16])
def test_learned_sinusoid_layout_and_planted_errors(half):
    g = _gen(half)
    t = torch.tensor([0.0, 1.0, 0.25, 0.7312])
    w = torch.randn(half, generator=g)
    ref = G.learned_sinusoid(t, w)
    f32 = G.learned_sinusoid(t, w, dtype=torch.float32)
    assert ref.shape == (4, 2 * half + 1)
    assert torch.equal(f32[:, 0], t)
    assert torch.allclose(ref[:, 1:half + 1], torch.sin(2 * math.pi * t.double()[:, None] * w.double()[None]))
    margin = _emb_margin(f32, ref, t)

    def ok(got):
        return all(float((got[i].double() - ref[i]).abs().max()) <= margin[float(t[i])] for i in range(len(t)))
    assert ok(f32)
    swapped = torch.cat([f32[:, :1], f32[:, half + 1:], f32[:, 1:half + 1]], dim=1)
    assert not ok(swapped)


def test_rows_copy_reference_and_a_written_skipped_row():
    g = _gen(5)
    src = torch.randn(9, 6, generator=g)
    dst = torch.full((12, 8), -7.0)
    smap = torch.tensor([3, -1, 0, 8, 2], dtype=torch.int32)
    dmap = torch.tensor([11, 4, -1, 0, 5], dtype=torch.int32)
    out, hit = G.rows_copy(src, dst, 5, smap, dmap, C=5)
    assert hit.nonzero().flatten().tolist() == [0, 5, 11]
    assert torch.equal(out[11, :5], src[3, :5]) and torch.equal(out[0, :5], src[8, :5]) and torch.equal(out[5, :5], src[2, :5])
    assert bool((out[~hit] == -7.0).all()) and bool((out[:, 5:] == -7.0).all())
    # what the GPU test asserts is bit-equality with this result: a kernel that also wrote the skipped i = 1 differs
    leaked = out.clone()
    leaked[4, :5] = src[0, :5]
    assert not torch.equal(leaked, out)
    out2, hit2 = G.rows_copy(src, dst, 4)
    assert torch.equal(out2[:4, :6], src[:4]) and int(hit2.sum()) == 4


@pytest.mark.parametrize('alpha', [0.9, 1e-3, 1e-9, 0.0])
@pytest.mark.parametrize('n', [1, 257])
def test_float32_ddim_eps_passes_and_a_missing_clamp_fails(alpha, n):
    g = _gen(7)
    x, eps = torch.randn(n, generator=g), torch.randn(n, generator=g)
    coef = torch.tensor([alpha, 0.43, 0.95, 0.31])
    xn, Sn, x0, S0 = G.ddim_eps(x, eps, coef)
    f = G.ddim_eps(x, eps, coef, dtype=torch.float32)
    G.assert_close(f[2], x0, S0, G.DDIM_EPS_C_X0, 'x0')
    G.assert_close(f[0], xn, Sn, G.DDIM_EPS_C_X, 'x')
    if alpha < 1e-8:
        bad = G.ddim_eps(x, eps, coef, dtype=torch.float32, clamp=False)
        with pytest.raises(AssertionError):
            G.assert_close(bad[2], x0, S0, G.DDIM_EPS_C_X0, 'x0 without the clamp')
        with pytest.raises(AssertionError):
            G.assert_close(bad[0], xn, Sn, G.DDIM_EPS_C_X, 'x without the clamp')
    if alpha >= 1e-3:                                              # (below, x0 alpha_next is 1e8 times the other term)
        with pytest.raises(AssertionError):                        # eps sigma_next dropped
            G.assert_close((x0 * coef[2].double()).float(), xn, Sn, G.DDIM_EPS_C_X, 'dropped term')


@pytest.mark.parametrize('alpha,sd', [(0.9, 0.2), (1e-3, 0.0), (1e-9, 0.2)])
@pytest.mark.parametrize('with_noise', [True, False])
def test_float32_ddim_x0_passes_and_a_dropped_term_fails(alpha, sd, with_noise):
    g = _gen(8)
    x, x0, noise = (torch.randn(257, generator=g) for _ in range(3))
    noise = noise if with_noise else None
    coef = torch.tensor([alpha, 0.37, 0.95, sd])
    ref, S = G.ddim_x0(x, x0, noise, coef)
    G.assert_close(G.ddim_x0(x, x0, noise, coef, dtype=torch.float32)[0], ref, S, G.DDIM_X0_C, 'x')
    if noise is None and sd != 0 and alpha >= 1e-3:
        with pytest.raises(AssertionError):                        # noise == NULL must mean "no noise term"
            G.assert_close(G.ddim_x0(x, x0, torch.ones(257), coef)[0].float(), ref, S, G.DDIM_X0_C, 'noise read')
    if alpha >= 1e-3:                                              # (below, x / alpha is 1e8 times the other terms)
        with pytest.raises(AssertionError):
            G.assert_close((ref - coef[2].double() * coef[1].double() * x0.double()).float(), ref, S, G.DDIM_X0_C,
                           'c x0 dropped')


def test_assert_close_rejects_nan_and_is_elementwise():
    ref = torch.tensor([1e6, 1e-6], dtype=torch.float64)
    S = ref.abs()
    G.assert_close(ref.float(), ref, S, 1.0)
    with pytest.raises(AssertionError):
        G.assert_close(torch.tensor([1e6, float('nan')]), ref, S, 1.0)
    with pytest.raises(AssertionError):                            # 1e-7 is nothing next to 1e6, and 10 % of the small one
        G.assert_close(torch.tensor([1e6, 1.1e-6]), ref, S, 4.0)
