"""The dense levels' 27-tap tables and their reverse, one entry point at a time: ofx_grid_conv_table (csrc/ofx_dense.hip) in
its three modes against the plain-loop tables of tests/gridtab_oracle.py at depths 0 .. 3, batch 1 and 3 and three
paddings; ofx_table_reverse_count -> ops.scan_i32 -> ofx_table_reverse_fill (csrc/ofx_graph.hip) against the brute-force
reverse CSR, whose segments must come back in ascending row order (the order that fixes the summation of the dense
convolutions' dx), on those tables and on hand-made ones with 1 and 7 taps, out-of-range entries on both sides and a
40-row segment; empty calls and refusals.  tests/test_gridtab_oracle.py checks the oracle against torch's conv3d on the
host."""
import pytest
import torch

import gridtab_oracle as T
from test_gpu_fullwidth import dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

ISENT = -77777                                     # int32 outputs
FSENT = -12345.678                                 # rev_w
GUARD = 16                                         # sentinel elements on either side of every output

CASES = [(mode, d, B) for mode, depths in ((0, (0, 1, 2, 3)), (1, (0, 1, 2)), (2, (1, 2, 3))) for d in depths for B in (1, 3)]


def _guarded(n, value, dtype):
    """(buffer, window): n elements between two GUARD-element sentinel runs (n = 0: an empty window, a real pointer)."""
    buf = torch.full((n + 2 * GUARD,), value, dtype=dtype, device=dev())
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, value, what):
    g = torch.cat([buf[:GUARD], buf[GUARD + n:]]).cpu()
    assert torch.equal(g, torch.full_like(g, value)), what + ': wrote outside its output'


def _device_reverse(tab, n_in):
    """count -> scan -> fill on the device for the tap table `tab` [n_out, ndir] (device, contiguous).  Returns host
    (rev_cnt, rev_ptr, rev_row, rev_w)."""
    from octfusion_amd import _lib, ops
    from octfusion_amd._lib import ptr, stream
    n_out, ndir = tab.shape
    nseg = n_in * ndir
    cbuf, cnt = _guarded(nseg, ISENT, torch.int32)
    _lib.call('ofx_table_reverse_count', ptr(tab), n_out, ndir, n_in, ptr(cnt), stream())
    rev_ptr = ops.scan_i32(cnt.contiguous())
    E = int(rev_ptr[-1])
    cubuf, cursor = _guarded(nseg, ISENT, torch.int32)
    rbuf, rev_row = _guarded(E, ISENT, torch.int32)
    wbuf, rev_w = _guarded(E, FSENT, torch.float32)
    _lib.call('ofx_table_reverse_fill', ptr(tab), n_out, ndir, n_in, ptr(rev_ptr), ptr(cursor), rbuf.data_ptr() + 4 * GUARD,
              wbuf.data_ptr() + 4 * GUARD, stream())
    torch.cuda.synchronize()
    for buf, n, val, name in ((cbuf, nseg, ISENT, 'rev_cnt'), (cubuf, nseg, ISENT, 'cursor'), (rbuf, E, ISENT, 'rev_row'),
                              (wbuf, E, FSENT, 'rev_w')):
        _guards_intact(buf, n, val, name)
    assert torch.equal(cursor, cnt), 'the fill placed another number of entries than the count found'
    return cnt.cpu(), rev_ptr.cpu(), rev_row.cpu(), rev_w.cpu()


def _check_reverse(tab_host, tab_dev, n_in, what):
    cnt, ptr_, row = T.reverse(tab_host, n_in)
    gcnt, gptr, grow, gw = _device_reverse(tab_dev, n_in)
    assert torch.equal(gcnt, cnt), what + ': rev_cnt'
    assert torch.equal(gptr, ptr_), what + ': rev_ptr'
    assert torch.equal(grow, row), what + ': rev_row (ascending inside each segment)'
    assert torch.equal(gw, torch.ones(row.numel())), what + ': rev_w'
    return cnt


@pytest.mark.parametrize('mode,depth_out,B', CASES, ids=['mode%d-d%d-B%d' % c for c in CASES])
def test_table_and_reverse(mode, depth_out, B):
    from octfusion_amd import _lib, ops
    from octfusion_amd._lib import ptr, stream
    n_in, n_out = T.n_in(mode, depth_out, B), B * 8 ** depth_out
    for pad in (-1, n_in, 123456789):
        ref = T.table(mode, depth_out, B, pad)
        got = ops.grid_conv_table(mode, depth_out, B, dev(), pad=pad)
        assert got.shape == ref.shape and torch.equal(got.cpu(), ref), (mode, depth_out, B, pad)
        buf, win = _guarded(n_out * 27, ISENT, torch.int32)                # the C ABI, for the elements next to the table
        _lib.call('ofx_grid_conv_table', mode, depth_out, B, pad, ptr(win), stream())
        torch.cuda.synchronize()
        _guards_intact(buf, n_out * 27, ISENT, 'ofx_grid_conv_table')
        assert torch.equal(win.cpu().view(n_out, 27), ref)
        cnt = _check_reverse(ref, got, n_in, 'mode %d depth %d B %d pad %d' % (mode, depth_out, B, pad))
    if mode == 2:                                                          # several output rows name one (source row, tap)
        assert int(cnt.max()) > 1
    else:
        assert int(cnt.max()) == 1


@pytest.mark.parametrize('ndir', [1, 7])
def test_hand_made_tables(ndir):
    """300 rows (more than one block of entries) over 50 sources: entries below 0, at n_in, above it and far above it mixed
    in, and one (source, tap) named by 40 rows scattered over the table -- a long segment for the insertion sort, filled
    in whatever order the atomics land.  That order is the hardware's: where it happens to be ascending already a missing
    sort goes unseen, so the long segment is a likely detector of a broken sort, not a certain one, and a pass does not
    prove that the sort ran."""
    n_out, n_in = 300, 50
    g = torch.Generator().manual_seed(ndir)
    tab = torch.randint(-3, n_in + 3, (n_out, ndir), generator=g, dtype=torch.int32)
    tab[torch.randperm(n_out, generator=g)[:20], ndir - 1] = 123456789
    tab[:, 0][tab[:, 0] == 5] = 6
    rows40 = torch.randperm(n_out, generator=g)[:40]
    tab[rows40, 0] = 5
    assert int((tab < 0).sum()) > 0 and int((tab == n_in).sum()) > 0 and int((tab == 123456789).sum()) > 0
    cnt = _check_reverse(tab, tab.to(dev()), n_in, 'hand-made ndir %d' % ndir)
    assert int(cnt[5 * ndir]) == 40 == int(cnt.max())


def test_empty_calls_touch_nothing():
    """n_in == 0: count and fill return at once, every output untouched.  n_out == 0: the fill returns at once with its
    outputs untouched; the count does write, it zeroes rev_cnt -- no output row names any source, and zero is the count
    the scan that follows needs."""
    from octfusion_amd import _lib
    from octfusion_amd._lib import ptr, stream
    tab = torch.zeros(8, 7, dtype=torch.int32, device=dev())
    cnt = torch.full((56,), ISENT, dtype=torch.int32, device=dev())
    cur = torch.full((56,), ISENT, dtype=torch.int32, device=dev())
    row = torch.full((56,), ISENT, dtype=torch.int32, device=dev())
    w = torch.full((56,), FSENT, device=dev())
    rev_ptr = torch.zeros(57, dtype=torch.int32, device=dev())
    same = lambda t, v: torch.equal(t.cpu(), torch.full_like(t, v).cpu())              # noqa: E731
    _lib.call('ofx_table_reverse_count', ptr(tab), 8, 7, 0, ptr(cnt), stream())
    _lib.call('ofx_table_reverse_fill', ptr(tab), 8, 7, 0, ptr(rev_ptr), ptr(cur), ptr(row), ptr(w), stream())
    _lib.call('ofx_table_reverse_fill', ptr(tab), 0, 7, 8, ptr(rev_ptr), ptr(cur), ptr(row), ptr(w), stream())
    torch.cuda.synchronize()
    assert same(cnt, ISENT) and same(cur, ISENT) and same(row, ISENT) and same(w, FSENT)
    _lib.call('ofx_table_reverse_count', ptr(tab), 0, 7, 8, ptr(cnt), stream())
    torch.cuda.synchronize()
    assert same(cnt, 0)


def test_refusals():
    from octfusion_amd import _lib
    from octfusion_amd._lib import ptr, stream
    tab = torch.full((8 * 27,), ISENT, dtype=torch.int32, device=dev())
    for mode, depth, B, p in ((3, 1, 1, ptr(tab)), (-1, 1, 1, ptr(tab)), (0, 9, 1, ptr(tab)), (0, -1, 1, ptr(tab)),
                              (2, 0, 1, ptr(tab)), (0, 1, 0, ptr(tab)), (0, 1, 1, None)):
        with pytest.raises(_lib.OfxError, match='invalid argument'):
            _lib.call('ofx_grid_conv_table', mode, depth, B, -1, p, stream())
    nbr = torch.zeros(8, 7, dtype=torch.int32, device=dev())
    cnt = torch.full((56,), ISENT, dtype=torch.int32, device=dev())
    cur = torch.full((56,), ISENT, dtype=torch.int32, device=dev())
    row = torch.full((56,), ISENT, dtype=torch.int32, device=dev())
    w = torch.full((56,), FSENT, device=dev())
    rev_ptr = torch.zeros(57, dtype=torch.int32, device=dev())
    for args in ((ptr(nbr), 8, 0, 8, ptr(cnt)), (None, 8, 7, 8, ptr(cnt)), (ptr(nbr), 8, 7, 8, None), (ptr(nbr), -1, 7, 8, ptr(cnt)),
                 (ptr(nbr), 8, 7, -1, ptr(cnt))):
        with pytest.raises(_lib.OfxError, match='invalid argument'):
            _lib.call('ofx_table_reverse_count', *args, stream())
    good = (ptr(nbr), 8, 7, 8, ptr(rev_ptr), ptr(cur), ptr(row), ptr(w))
    bad = [good[:2] + (0,) + good[3:], good[:1] + (-1,) + good[2:], good[:3] + (-1,) + good[4:]]
    bad += [good[:i] + (None,) + good[i + 1:] for i in (0, 4, 5, 6, 7)]
    for args in bad:
        with pytest.raises(_lib.OfxError, match='invalid argument'):
            _lib.call('ofx_table_reverse_fill', *args, stream())
    torch.cuda.synchronize()
    for t, v in ((tab, ISENT), (cnt, ISENT), (cur, ISENT), (row, ISENT)):
        assert torch.equal(t.cpu(), torch.full_like(t, v).cpu())
    assert torch.equal(w.cpu(), torch.full_like(w, FSENT).cpu())
