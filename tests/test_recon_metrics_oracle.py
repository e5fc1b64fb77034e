"""CPU checks of the float64 oracle of the reconstruction scores (tests/recon_metrics_oracle.py) on cases computed by
hand, of the packed-bit order against numpy.packbits, and of recon_metrics' refusal to run without a device."""
import math

import numpy as np
import pytest
import torch

import recon_metrics_oracle as MO


def test_nearest_two_points():
    q = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 2.0]])
    t = np.array([[0.0, 3.0, 4.0], [1.0, 2.0, 0.0]])
    d2, ix = MO.nearest(q, t)                     # |q0 - t|^2 = 25, 5;  |q1 - t|^2 = 6, 4
    assert d2.tolist() == [5.0, 4.0] and ix.tolist() == [1, 1] and ix.dtype == np.int32
    d2, ix = MO.nearest(t, q)
    assert d2.tolist() == [6.0, 4.0] and ix.tolist() == [1, 1]
    d2, ix = MO.nearest(q, np.zeros((0, 3)))
    assert np.isinf(d2).all() and ix.tolist() == [-1, -1]
    d2, ix = MO.nearest(np.zeros((0, 3)), t)
    assert d2.shape == (0,) and ix.shape == (0,)


def test_nearest_duplicated_target_takes_the_lowest_index():
    t = np.array([[5.0, 5.0, 5.0], [1.0, 0.0, 0.0], [9.0, 9.0, 9.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])
    d2, ix = MO.nearest(np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]]), t, chunk=1)
    assert d2.tolist() == [0.0, 1.0] and ix.tolist() == [1, 1]      # the copy at 3 and the mirror point at 4 lose
    assert MO.dist2_to(np.array([[0.0, 0.0, 0.0]]), t, np.array([4])).tolist() == [1.0]


def test_scores_by_hand_with_a_threshold_exactly_at_a_distance():
    """gt = two points on the x axis, pred = the same moved by 0.5 and 0.25 along y; normals parallel, opposite and at
    60 degrees.  Distances 0.5 and 0.25 both ways; a threshold equal to a distance counts (<=)."""
    gt = (np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0]]), np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]]))
    pred = (np.array([[0.0, 0.5, 0.0], [4.0, 0.25, 0.0]]),
            np.array([[0.0, 0.0, -1.0], [0.0, math.sqrt(0.75), 0.5]]))
    s = MO.surface_scores(gt, pred, thresholds=(0.125, 0.25, 0.5, 0.2499999))
    assert s['completeness'] == s['accuracy'] == s['chamfer_l1'] == 0.375
    assert s['completeness2'] == s['accuracy2'] == s['chamfer_l2'] == (0.25 + 0.0625) / 2
    assert s['normals_completeness'] == s['normals_accuracy'] == s['normal_consistency'] == 0.75
    assert s['recall'] == s['precision'] == [0.0, 0.5, 1.0, 0.0]
    assert s['fscore'] == [0.0, 0.5, 1.0, 0.0]                      # P + R == 0 gives 0, not a division by zero
    # an asymmetric pair: every pred point is near gt (precision 1) but half of gt is far from pred (recall 1/2)
    one = (pred[0][:1], pred[1][:1])
    s = MO.surface_scores(gt, one, thresholds=(1.0,))
    assert s['recall'] == [0.5] and s['precision'] == [1.0] and s['fscore'] == [2 * 0.5 / 1.5]
    assert s['accuracy'] == 0.5 and s['completeness'] == (0.5 + math.sqrt(16.25)) / 2


def test_bit_order_is_numpy_packbits():
    rng = np.random.default_rng(5)
    for n in (1, 7, 8, 9, 61):
        occ = rng.integers(0, 2, n).astype(bool)
        assert np.array_equal(MO.unpack_bits(np.packbits(occ), n), occ)
    assert MO.unpack_bits(np.array([0b10000001, 0b01000000], np.uint8), 10).tolist() == \
        [True, False, False, False, False, False, False, True, False, True]


def test_iou_by_hand_and_empty_union():
    values = np.array([-1.0, -0.5, 0.0, 0.5, -2.0, 3.0, -0.25, 1.0, -1.0, 2.0], np.float32)    # 10 points: not a byte multiple
    occ = np.array([1, 0, 1, 0, 1, 1, 0, 0, 0, 1], bool)
    bits = np.packbits(occ)
    bits[-1] |= 0b00111111                           # garbage in the padding bits must not count
    # pred = value < 0 (strict: the 0.0 is outside): points 0, 1, 4, 6, 8;  gt: 0, 2, 4, 5, 9
    assert MO.occupancy_iou(values, bits) == (2 / 8, 2, 8)
    assert MO.occupancy_iou(values, bits, level=0.25) == (3 / 8, 3, 8)
    assert MO.occupancy_iou(np.ones(10, np.float32), np.zeros(2, np.uint8)) == (None, 0, 0)


def test_driver_flags():
    from octfusion_amd import reconstruct as R, recon_metrics
    a = R.parse_args(['--input', 'x', '--out', 'y'])
    assert a.metrics is False and a.occupancy is False and tuple(a.thresholds) == recon_metrics.THRESHOLDS
    a = R.parse_args(['--input', 'x', '--out', 'y', '--metrics', '--thresholds', '0.02', '0.05', '--occupancy'])
    assert a.metrics is True and a.occupancy is True and a.thresholds == [0.02, 0.05]
    with pytest.raises(ValueError):
        R.parse_args(['--input', 'x', '--out', 'y', '--metrics', '--thresholds', '0'])


@pytest.mark.skipif(torch.cuda.is_available(), reason='a device is present')
def test_no_cpu_path():
    from octfusion_amd import recon_metrics
    from octfusion_amd._lib import OfxError
    a = torch.zeros(1, 4, 3)
    with pytest.raises(OfxError):
        recon_metrics.nearest(a, a)
    with pytest.raises(OfxError):
        recon_metrics.surface_scores((a[0], a[0]), (a[0], a[0]))
    with pytest.raises(OfxError):
        recon_metrics.occupancy_iou(lambda p: p[:, 0], a[0], np.zeros(1, np.uint8), 0.5)
