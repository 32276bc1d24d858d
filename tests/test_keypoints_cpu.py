"""Keypoints without a GPU (imm_amd/keypoints.py): the regressor's fit against scikit-learn and the evaluation code, its file, the
box checks and the geometry that maps the S x S frame back to source pixels."""
import numpy as np
import pytest

from imm_amd.eval import eval_imm
from imm_amd import keypoints as KP


def fixture_tensors(n, K, M, seed, S=128):
    """Landmarks in [-1, 1] and annotated points that depend on them linearly plus noise (a well-posed fit)."""
    rng = np.random.RandomState(seed)
    mu = rng.uniform(-0.8, 0.8, size=(n, K, 2)).astype(np.float32)
    A = rng.standard_normal((2 * K, 2 * M)) * 0.3
    pts = (((mu + 1) / 2.0 * S).reshape(n, -1) @ A + 20.0 + rng.standard_normal((n, 2 * M))).reshape(n, M, 2)
    return {'gauss_yx': mu, 'future_landmarks': pts.astype(np.float32)}


@pytest.mark.parametrize('bias', [False, True], ids=['no_bias', 'bias'])
def test_fit_equals_sklearn_and_regress_landmarks(bias):
    import sklearn.linear_model
    train, test = fixture_tensors(60, 10, 5, 0), fixture_tensors(17, 10, 5, 1)
    reg = KP.LandmarkRegressor.fit(train, [128, 128], bias)
    x, y = eval_imm.convert_landmarks(train, [128, 128])
    ref = sklearn.linear_model.Ridge(alpha=0.0, fit_intercept=bias).fit(x, y)
    np.testing.assert_array_equal(reg.coef, ref.coef_)
    np.testing.assert_array_equal(reg.intercept, np.broadcast_to(ref.intercept_, (10,)))
    assert (reg.K, reg.M, reg.S, reg.bias) == (10, 5, 128, bias)
    assert reg.labels == KP.MAFL_LABELS
    if not bias:
        assert not reg.intercept.any()
    # host predict == the evaluation code's regression, bit for bit
    np.testing.assert_array_equal(reg.predict(test['gauss_yx']), eval_imm.regress_landmarks(train, test, [128, 128], bias))
    # the epilogue's f32 weights are the transposed coefficients
    w, b = reg.epilogue_weights()
    assert w.shape == (20, 10) and b.shape == (10,) and w.dtype == np.float32
    np.testing.assert_array_equal(w, reg.coef.T.astype(np.float32))


def test_save_load_round_trip_and_mismatch(tmp_path):
    train = fixture_tensors(40, 6, 5, 2, S=96)
    reg = KP.LandmarkRegressor.fit(train, 96, True, dataset='mafl', checkpoint='logs/model.ckpt-100')
    path = str(tmp_path / 'reg.npz')
    reg.save(path)

    class Det(object):
        def __init__(self, K, S):
            self.K, self.S = K, S

    back = KP.LandmarkRegressor.load(path, detector=Det(6, 96))
    np.testing.assert_array_equal(back.coef, reg.coef)
    np.testing.assert_array_equal(back.intercept, reg.intercept)
    assert back.coef.dtype == np.float64
    assert (back.K, back.M, back.S, back.bias, back.labels, back.dataset, back.checkpoint) == \
        (6, 5, 96, True, KP.MAFL_LABELS, 'mafl', 'logs/model.ckpt-100')
    np.testing.assert_array_equal(back.predict(train['gauss_yx']), reg.predict(train['gauss_yx']))
    for K, S in ((7, 96), (6, 128)):
        with pytest.raises(ValueError):
            KP.LandmarkRegressor.load(path, detector=Det(K, S))
    np.savez(str(tmp_path / 'other.npz'), coef=reg.coef)
    with pytest.raises(ValueError):
        KP.LandmarkRegressor.load(str(tmp_path / 'other.npz'))


def test_bad_boxes_and_too_many_points_are_rejected():
    ok = KP.check_boxes([(0, -5, -5, 50, 40), (1, 10, 10, 11, 11), (0, 100, 100, 200, 300)], 2)
    assert ok.dtype == np.int32 and ok.shape == (3, 5)
    np.testing.assert_array_equal(KP.check_boxes([(1, 2, 3, 4), (5, 6, 7, 8)], 2), [[0, 1, 2, 3, 4], [1, 5, 6, 7, 8]])
    for bad in ([(0, 10, 0, 10, 20)],          # y1 <= y0
                [(0, 0, 10, 20, 5)],           # x1 <= x0
                [(2, 0, 0, 10, 10)],           # image index out of range
                [(-1, 0, 0, 10, 10)],
                [(1, 2, 3, 4)],                # four-value boxes, not one per image
                [(0, 1, 2)],
                []):
        with pytest.raises(ValueError):
            KP.check_boxes(bad, 2)
    rng = np.random.RandomState(0)
    reg = KP.LandmarkRegressor(rng.standard_normal((34, 20)), np.zeros(34), 10, 128, False)       # M = 17
    assert reg.M == 17
    with pytest.raises(ValueError):
        reg.epilogue_weights()
    import torch
    from imm_amd import ops
    z = lambda *s: torch.zeros(*s)
    with pytest.raises(ValueError):
        ops.keypoint_desc(z(20, 34), z(34), z(4, 4), z(4, 17, 2), 128)
    assert ops.keypoint_desc(z(20, 32), z(32), z(4, 4), z(4, 16, 2), 128).m == 16


def test_geometry_known_answers():
    from imm_amd.datasets.impair_dataset import ImagePairDataset
    S = 128
    boxes = KP.check_boxes([(0, 30, 40, 230, 190), (0, -20, 7, 44, 71), (1, 0, 0, 300, 250)], 2)
    geom = KP.box_geometry(boxes, S)
    assert geom.dtype == np.float32
    np.testing.assert_array_equal(geom[0], np.float32([30, 40, 200.0 / 128, 150.0 / 128]))
    np.testing.assert_array_equal(KP.image_geometry([(300, 250)], S)[0], geom[2])
    # a keypoint at S-frame p maps to y0 + p * h_box / S
    p = np.array([[[0.0, 0.0], [64.0, 64.0], [128.0, 128.0], [13.5, 101.25]]] * 3)
    src = KP.to_source_pixels(p, geom)
    for b, (_i, y0, x0, y1, x1) in enumerate(boxes):
        np.testing.assert_allclose(src[b, :, 0], y0 + p[b, :, 0] * (y1 - y0) / S, rtol=0, atol=1e-4)
        np.testing.assert_allclose(src[b, :, 1], x0 + p[b, :, 1] * (x1 - x0) / S, rtol=0, atol=1e-4)
    np.testing.assert_array_equal(src[:, 0], geom[:, :2])
    np.testing.assert_allclose(src[:, 2], boxes[:, 3:].astype(np.float64), rtol=0, atol=1e-4)
    # composed with the datasets' _resize_points (box pixels -> S x S frame), it is the identity on source pixels
    ds = ImagePairDataset.__new__(ImagePairDataset)
    rng = np.random.RandomState(3)
    for b, (_i, y0, x0, y1, x1) in enumerate(boxes):
        q = np.stack([rng.uniform(y0, y1, 8), rng.uniform(x0, x1, 8)], axis=1).astype(np.float32)
        in_frame = ds._resize_points(q - np.float32([y0, x0]), [y1 - y0, x1 - x0], [S, S])
        np.testing.assert_allclose(KP.to_source_pixels(in_frame[None], geom[b:b + 1])[0], q, rtol=0, atol=1e-3)


def test_square_box_is_the_datasets_fit_bbox():
    from imm_amd.datasets.impair_dataset import ImagePairDataset
    for box in ((10, 20, 110, 70), (5, 5, 25, 95), (0, 0, 50, 50)):
        sq = KP.square_box(box)
        assert sq.dtype == np.int32
        np.testing.assert_array_equal(sq, ImagePairDataset._fit_bbox(None, box, (1, 1)))
        h, w = sq[2] - sq[0], sq[3] - sq[1]
        assert abs(int(h) - int(w)) <= 1
