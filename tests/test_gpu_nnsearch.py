"""GPU checks of the nearest-neighbour search (csrc/ofx_nnsearch.hip, ofx_nn_search / recon_metrics.nearest) against the
float64 oracle tests/recon_metrics_oracle.py.

Exactness.  The lattice cases use coordinates k / 64, |k| <= 128: a difference is an integer / 64 below 2^9 / 64, a
square an integer / 4096 below 2^18 / 4096 and the sum of three below 2^20 / 4096 -- all exact in fp32, fused or not --
so the device must equal the float64 oracle bit for bit, index included (ties go to the lowest index).
Random fp32 clouds.  A difference of two fp32 numbers is rounded once (relative 2^-24), its square carries twice that
plus a rounding, and the two fused additions add one rounding each on non-negative terms: under 5 * 2^-24 = 3e-7
relative on the squared distance, so 1e-6 bounds both the reported distance against the float64 distance of the
reported index, and that distance against the float64 minimum (the device may prefer a target whose float64 distance is
larger by no more than the error of the comparison).
Sizes.  Read from the library: the queries a block owns (ofx_nn_search_qpass) and the LDS tile (ofx_nn_search_tile),
each hit one below, exactly and one above, next to one point and to a target cloud of a dozen tiles, which the
automatic geometry cuts into a dozen slices."""
import numpy as np
import pytest
import torch

import recon_metrics_oracle as MO
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _consts():
    from octfusion_amd import _lib
    L = _lib.lib()
    return L.ofx_nn_search_qpass(), L.ofx_nn_search_tile()


def _lattice(n, seed, dup=0):
    """[n, 3] float32 with coordinates k / 64 in [-2, 2]; the last `dup` rows repeat earlier ones."""
    rng = np.random.default_rng(seed)
    p = rng.integers(-128, 129, (n, 3)).astype(np.float32) / np.float32(64)
    if dup:
        p[n - dup:] = p[rng.integers(0, n - dup, dup)]
    return p


def _search(q, t, splits=0):
    from octfusion_amd import recon_metrics as RM
    d2, ix = RM.nearest([torch.from_numpy(q)], [torch.from_numpy(t)], splits=splits)
    assert d2[0].dtype == torch.float32 and ix[0].dtype == torch.int32 and d2[0].shape == ix[0].shape == (len(q),)
    return d2[0].cpu().numpy(), ix[0].cpu().numpy()


def _cases():
    return ['one', 'below', 'exact', 'above', 'tile_tail', 'slices']


def _sizes(name):
    QP, TILE = _consts()
    return {'one': (1, 1), 'below': (QP - 1, TILE - 1), 'exact': (QP, TILE), 'above': (QP + 1, TILE + 1),
            'tile_tail': (67, 2 * TILE + 1), 'slices': (QP + 452, 12 * TILE - 5)}[name]


@pytest.mark.parametrize('name', _cases())
def test_lattice_clouds_equal_the_oracle_bitwise(name):
    from octfusion_amd import _lib
    nq, nt = _sizes(name)
    q = _lattice(nq, 11)
    t = _lattice(nt, 12, dup=nt // 5)                 # a fifth of the targets are copies of earlier ones
    if nt > 1:
        q[: nq // 2] = t[np.random.default_rng(13).integers(0, nt, nq // 2)]      # half the queries hit a target
    want_d, want_i = MO.nearest(q, t)
    if name == 'slices':
        assert _lib.lib().ofx_nn_search_splits(1, nq, nt) >= 4
    if name in ('above', 'slices'):
        assert MO.tied_queries(q, t) > nq // 20                       # the tie rule is exercised
    for splits in (0, 1, 3):
        got_d, got_i = _search(q, t, splits)
        assert np.array_equal(got_i, want_i), (splits, int((got_i != want_i).sum()))
        assert np.array_equal(got_d, want_d.astype(np.float32)), splits
        assert np.array_equal(got_d.astype(np.float64), want_d)


def test_ragged_batch_through_the_c_abi():
    """Five pairs of different sizes in one call, one with an empty target cloud (+inf, -1), one with an empty query
    cloud (nothing written); the output arrays sit inside larger sentinel-filled buffers, which stay intact."""
    from octfusion_amd import _lib
    QP, TILE = _consts()
    sizes = [(700, TILE + 476), (300, 0), (0, 400), (QP + 452, 90), (1, 3 * TILE - 72)]
    qs = [_lattice(n, 20 + k) for k, (n, _) in enumerate(sizes)]
    ts = [_lattice(m, 40 + k, dup=m // 4) for k, (_, m) in enumerate(sizes)]
    nq, nt = [n for n, _ in sizes], [m for _, m in sizes]
    Q, PAD = sum(nq), 64
    q = torch.from_numpy(np.concatenate(qs)).to(dev())
    t = torch.from_numpy(np.concatenate(ts)).to(dev())
    offs = torch.tensor(np.concatenate([np.cumsum([0] + nq), np.cumsum([0] + nt)]), dtype=torch.int64).to(dev())
    ws = torch.empty(_lib.lib().ofx_nn_search_ws_bytes(Q), dtype=torch.uint8, device=dev())
    for splits in (0, 1, 3):
        d2 = torch.full((Q + 2 * PAD,), -7.0, dtype=torch.float32, device=dev())
        ix = torch.full((Q + 2 * PAD,), -7, dtype=torch.int32, device=dev())
        _lib.call('ofx_nn_search', q.data_ptr(), offs.data_ptr(), t.data_ptr(), offs[len(sizes) + 1:].data_ptr(),
                  len(sizes), Q, max(nq), max(nt), splits, ws.data_ptr(), d2[PAD:].data_ptr(), ix[PAD:].data_ptr(),
                  _lib.stream())
        d2, ix = d2.cpu().numpy(), ix.cpu().numpy()
        for pad in (slice(0, PAD), slice(PAD + Q, None)):
            assert (d2[pad] == -7.0).all() and (ix[pad] == -7).all()
        at = PAD
        for k in range(len(sizes)):
            want_d, want_i = MO.nearest(qs[k], ts[k])
            assert np.array_equal(ix[at:at + nq[k]], want_i), (splits, k)
            assert np.array_equal(d2[at:at + nq[k]], want_d.astype(np.float32)), (splits, k)
            at += nq[k]
        assert np.isinf(d2[PAD + 700:PAD + 1000]).all() and (ix[PAD + 700:PAD + 1000] == -1).all()


def test_lists_stacked_batches_and_arguments():
    from octfusion_amd import _lib, recon_metrics as RM
    a = torch.from_numpy(_lattice(3 * 50, 60).reshape(3, 50, 3)).to(dev())
    b = torch.from_numpy(_lattice(3 * 70, 61).reshape(3, 70, 3)).to(dev())
    d2, ix = RM.nearest(a, b)
    assert d2.shape == ix.shape == (3, 50)
    dl, il = RM.nearest([a[0], a[1], a[2]], [b[0], b[1], b[2]])
    for k in range(3):
        want_d, want_i = MO.nearest(a[k].cpu().numpy(), b[k].cpu().numpy())
        assert torch.equal(d2[k], dl[k]) and torch.equal(ix[k], il[k])
        assert np.array_equal(ix[k].cpu().numpy(), want_i) and np.array_equal(d2[k].cpu().numpy().astype(np.float64), want_d)
    # no queries at all: nothing to launch; an empty list of pairs likewise
    e = torch.zeros(0, 3, device=dev())
    dl, il = RM.nearest([e], [b[0]])
    assert dl[0].shape == il[0].shape == (0,)
    assert RM.nearest([], []) == ([], [])
    with pytest.raises(ValueError):
        RM.nearest([a[0]], [b[0], b[1]])
    L = _lib.lib()
    x = torch.zeros(16, device=dev())
    p = x.data_ptr()
    assert L.ofx_nn_search(None, None, None, None, 0, 0, 0, 0, 0, None, None, None, None) == 0     # batch == 0
    assert L.ofx_nn_search(p, p, p, p, 1, 0, 0, 5, 0, None, p, p, None) == 0                       # Q == 0
    assert L.ofx_nn_search(p, p, p, p, 1, 1, 1, 2 ** 31, 0, p, p, p, None) != 0                    # idx would not fit
    assert L.ofx_nn_search(p, p, p, p, 1, 1, 1, 1, -1, p, p, p, None) != 0
    assert L.ofx_nn_search(p, p, p, p, 1, 1, 1, 1, 0, p, None, p, None) != 0
    assert L.ofx_nn_search(p, p, p, p, 1, 5, 5, 5000, 2, None, p, p, None) != 0                    # slices need ws


def _random_clouds():
    g = torch.Generator().manual_seed(77)
    QP, TILE = _consts()
    q = (torch.rand(QP + 900, 3, generator=g) - 0.5).numpy()
    t = (torch.rand(9 * TILE - 300, 3, generator=g) - 0.5).numpy()
    return q, t


def test_geometry_independence_and_repeats():
    q, t = _random_clouds()
    base = _search(q, t, 1)
    for splits in (3, 7, 0, 1, 0):
        got = _search(q, t, splits)
        assert np.array_equal(got[0].view(np.uint32), base[0].view(np.uint32)), splits
        assert np.array_equal(got[1], base[1]), splits


def test_random_clouds_within_fp32_rounding():
    q, t = _random_clouds()
    got_d, got_i = _search(q, t)
    want_d, _ = MO.nearest(q, t)
    assert got_i.min() >= 0 and got_i.max() < len(t)
    at = MO.dist2_to(q, t, got_i)
    print('max (d64[idx] - min64) / min64 = %.3g' % ((at - want_d) / want_d).max())
    print('max |dist2 - d64[idx]| / d64[idx] = %.3g' % (np.abs(got_d - at) / at).max())
    assert (at <= want_d * (1 + 1e-6)).all()
    assert (np.abs(got_d.astype(np.float64) - at) <= 1e-6 * at).all()


def test_a_cloud_against_itself():
    q, _ = _random_clouds()
    assert len(np.unique(q, axis=0)) == len(q)
    for splits in (0, 1, 3):
        d2, ix = _search(q, q, splits)
        assert (d2 == 0).all() and np.array_equal(ix, np.arange(len(q), dtype=np.int32))
