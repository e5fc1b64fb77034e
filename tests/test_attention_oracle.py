"""tests/attention_oracle.py on the host: torch's fp32 evaluation of QKVAttention stays under HALF the elementwise bound on
every (shape, input kind) tests/test_gpu_attention_entry.py uses; errors of the kind the kernel can make (a key dropped, a
padded key let in, a scale forgotten, the head layout misread, rows swapped, a wave's keys missing from the denominator) do
not stay under it on the inputs written to catch them; and the mirror of the launcher's arithmetic matches the envelope
the header states.  No GPU, no octfusion_amd."""
import pytest
import torch

import attention_oracle as A

torch.set_grad_enabled(False)

CASES = A.fwd_cases()
WORST = {}


def _ids(cases):
    return ['%d-%d-%d-%d-%s' % (s + (k,)) for s, k in cases]


def _softmax_out(s, v):
    """out [B, T, heads, ch] from scores [B, heads, T, S] and values [B, S, heads, ch]."""
    return torch.einsum('bhts,bshc->bthc', torch.softmax(s, dim=-1), v)


def _parts(qkv, B, T, heads):
    q, k, v, ch = A._qkv(qkv, B, T, heads, torch.float64)
    scale = ch ** -0.25
    return q, k, v, ch, scale, torch.einsum('bthc,bshc->bhts', q * scale, k * scale)


def _rejected(got, ref, bound):
    """Share of elements outside the bound."""
    return float(((got.reshape(ref.shape) - ref).abs() > bound).double().mean())


# ------------------------------------------------------------------------------------------------ honest arithmetic
@pytest.mark.parametrize('shape,kind', CASES, ids=_ids(CASES))
def test_fp32_evaluation_stays_under_half_the_bound(shape, kind):
    B, T, heads, ch = shape
    qkv = A.make(kind, *shape)
    ref, bound = A.forward(qkv, B, T, heads)
    assert bool((bound > 0).all()) and bool(torch.isfinite(bound).all())
    used = A.ratio(A.evaluate(qkv, B, T, heads, torch.float32), ref, bound)
    WORST[kind] = max(WORST.get(kind, 0.0), used)
    print('fp32 on the CPU uses %.3f of the bound at %r %s' % (used, shape, kind))
    assert used <= 0.5, (shape, kind, used)
    if kind == 'plain':           # a roundoff bound, not a tolerance: under 1e-3 of the largest value everywhere
        assert float(bound.max()) < 1e-3 * float(ref.abs().max())


def test_single_key_returns_the_values():
    shape = (2, 1, 2, 6)
    qkv = A.make('plain', *shape)
    ref, _ = A.forward(qkv, 2, 1, 2)
    assert torch.equal(ref, A.values(qkv, 2, 1, 2).double())


def test_input_kinds_put_the_scores_where_they_say():
    shape = (2, 100, 3, 40)
    for kind, lo, hi in (('offset', 60, 140), ('negative', -70, -5)):
        s = _parts(A.make(kind, *shape), 2, 100, 3)[5]
        assert lo < float(s.median()) < hi and float((s > lo).double().mean()) > 0.99, (kind, float(s.median()))
    for shp in A.FWD_SHAPES[1:]:
        s = _parts(A.make('lastkey', *shp), *shp[:3])[5]
        assert bool((s.argmax(dim=-1) == shp[1] - 1).all()), shp
    p = torch.softmax(_parts(A.make('peaked', *shape), 2, 100, 3)[5], dim=-1)
    assert float(p.max(dim=-1).values.median()) > 0.9


# ------------------------------------------------------------------------------------------------ planted errors
DROP = [(s, k) for s in A.FWD_SHAPES + A.LAYOUT_SHAPES if s[1] > 1 for k in ('plain', 'negative', 'lastkey', 'offset')]


@pytest.mark.parametrize('shape,kind', DROP, ids=_ids(DROP))
def test_last_real_key_dropped_is_rejected(shape, kind):
    B, T, heads, ch = shape
    qkv = A.make(kind, *shape)
    ref, bound = A.forward(qkv, B, T, heads)
    q, k, v, ch, scale, s = _parts(qkv, B, T, heads)
    got = _softmax_out(s[..., :T - 1], v[:, :T - 1])
    assert _rejected(got, ref, bound) > 0, (shape, kind)
    if kind == 'lastkey':
        assert _rejected(got, ref, bound) > 0.99


@pytest.mark.parametrize('shape', A.FWD_SHAPES, ids=lambda s: '%d-%d-%d-%d' % s)
def test_padded_key_admitted_is_rejected(shape):
    """One zero-score, zero-value key next to the real ones (what a staged-as-zero padded key is when the mask misses it)."""
    B, T, heads, ch = shape
    qkv = A.make('negative', *shape)
    ref, bound = A.forward(qkv, B, T, heads)
    q, k, v, ch, scale, s = _parts(qkv, B, T, heads)
    s1 = torch.cat([s, torch.zeros_like(s[..., :1])], dim=-1)
    v1 = torch.cat([v, torch.zeros_like(v[:, :1])], dim=1)
    assert _rejected(_softmax_out(s1, v1), ref, bound) > 0.99, shape


MULTI = [s for s in A.FWD_SHAPES + A.LAYOUT_SHAPES if s[1] > 1]


@pytest.mark.parametrize('shape', MULTI, ids=lambda s: '%d-%d-%d-%d' % s)
def test_scale_on_q_only_is_rejected(shape):
    B, T, heads, ch = shape
    qkv = A.make('plain', *shape)
    ref, bound = A.forward(qkv, B, T, heads)
    q, k, v, ch, scale, s = _parts(qkv, B, T, heads)
    assert _rejected(_softmax_out(s / scale, v), ref, bound) > 0, shape


@pytest.mark.parametrize('shape', [s for s in MULTI if s[2] > 1], ids=lambda s: '%d-%d-%d-%d' % s)
def test_whole_row_qkv_blocks_are_rejected(shape):
    """channel = {q | k | v} * C + head * ch instead of head * 3 ch + {q | k | v}."""
    B, T, heads, ch = shape
    qkv = A.make('plain', *shape)
    ref, bound = A.forward(qkv, B, T, heads)
    wrong = qkv.view(B * T, 3, heads, ch).permute(0, 2, 1, 3).reshape(B * T, 3 * heads * ch)
    assert _rejected(A.forward(wrong, B, T, heads)[0], ref, bound) > 0, shape


@pytest.mark.parametrize('shape', [s for s in MULTI if s[1] > 4], ids=lambda s: '%d-%d-%d-%d' % s)
def test_two_queries_swapped_are_rejected(shape):
    """Rows q and q + 4 of the last 32-query tile exchanged (the C/D layout's register-to-row map off by one group)."""
    B, T, heads, ch = shape
    qkv = A.make('plain', *shape)
    ref, bound = A.forward(qkv, B, T, heads)
    got = ref.clone().view(B, T, -1)
    got[:, [T - 5, T - 1]] = got[:, [T - 1, T - 5]]
    assert _rejected(got.view(B * T, -1), ref, bound) > 0, shape


@pytest.mark.parametrize('shape', [s for s in MULTI if s[1] >= 256], ids=lambda s: '%d-%d-%d-%d' % s)
def test_a_wave_missing_from_the_denominator_is_rejected(shape):
    """The split-keys combine with the last wave's tiles (a quarter of the keys) left out of the sum of exponentials."""
    B, T, heads, ch = shape
    qkv = A.make('plain', *shape)
    ref, bound = A.forward(qkv, B, T, heads)
    q, k, v, ch, scale, s = _parts(qkv, B, T, heads)
    e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    kept = 32 * sum(A.split_tiles(T)[:3])
    assert T // 2 < kept < T
    got = torch.einsum('bhts,bshc->bthc', e / e[..., :kept].sum(dim=-1, keepdim=True), v)
    assert _rejected(got, ref, bound) > 0.5, shape


# ------------------------------------------------------------------------------------------------ the launcher mirror
def test_path_mirror_matches_the_envelope():
    for ch, width, most in ((32, 32, 544), (64, 64, 288), (128, 128, 128), (1, 32, 544), (33, 64, 288), (65, 128, 128)):
        p = A.path(most, ch, 3 * ch)
        assert (p.width, p.accepted) == (width, True), (ch, p)
        assert not A.path(most + 1, ch, 3 * ch).accepted, (ch, most + 1)
        assert A.path(most - 31, ch, 3 * ch).accepted
    # the same numbers from the rule as the header states it
    for width, most in ((32, 544), (64, 288), (128, 128)):
        assert 2 * most * (width + 4) * 4 <= 160 * 1024 - 2048 < 2 * (most + 32) * (width + 4) * 4
    assert [A.path(T, 16, 48).split for T in (255, 256, 257)] == [False, True, True]
    assert not A.path(512, 16, 48, split_on=False).split
    assert A.path(64, 32, 96).staging == 'float4'
    assert A.path(64, 30, 90).staging == 'ch' and A.path(64, 30, 92, aligned=False).staging == 'ch'
    assert A.path(64, 32, 99).staging == 'pitch' and A.path(64, 32, 100, aligned=False).staging == 'base'
    assert A.path(64, 32, 104).staging == 'float4'
    assert A.path(64, 32, 96, ld_other=35).staging == 'pitch' and A.path(64, 32, 96, ld_other=36).staging == 'float4'
    assert A.split_tiles(257) == [2, 2, 2, 3] and A.split_tiles(256) == [2, 2, 2, 2] and A.split_tiles(530) == [4, 4, 4, 5]


def test_case_lists_reach_every_path():
    """The shapes of the GPU file, by the mirror: each width unsplit, 32 and 64 split, float4 and scalar-by-ch staging
    from the contiguous cases (the pitch and base triggers come from its layouts, at ch % 4 == 0)."""
    have = {A.path(T, ch, 3 * heads * ch)[:3] for B, T, heads, ch in A.FWD_SHAPES}
    for want in ((32, False, 'ch'), (32, False, 'float4'), (64, False, 'float4'), (128, False, 'float4'), (128, False, 'ch'),
                 (32, True, 'float4'), (64, True, 'float4')):
        assert want in have, want
    assert all(A.path(T, ch, 3 * heads * ch).accepted for B, T, heads, ch in A.FWD_SHAPES + A.LAYOUT_SHAPES)
    assert all(ch % 4 == 0 for B, T, heads, ch in A.LAYOUT_SHAPES)
    assert all(T <= 512 for B, T, heads, ch in A.BWD_SHAPES)


def test_backward_floor_is_small():
    """The fp32 CPU gradient against the float64 one: the floor the GPU file's criterion scales from is roundoff-sized."""
    for shape in ((3, 33, 2, 30), (1, 97, 1, 100)):
        B, T, heads, ch = shape
        for kind in A.BWD_KINDS:
            qkv = A.make(kind, *shape)
            dout = torch.randn(B * T, heads * ch, generator=torch.Generator().manual_seed(T))
            g64, g32 = A.backward(qkv, dout, B, T, heads)
            assert float((g32.double() - g64).abs().max()) <= 2e-5 * float(g64.abs().max()), (shape, kind)


def test_zz_worst_ratio():
    """(runs last in this module) the largest share of the bound that honest fp32 arithmetic used, per input kind."""
    print('fp32 on the CPU, worst |err| / bound per input kind: %r' % WORST)
    assert WORST and all(v <= 0.5 for v in WORST.values())
