"""Keypoints of a trained model: the annotated points of a face (MAFL / AFLW: the two eyes, the nose, the two mouth corners) regressed
from the model's K unsupervised landmarks, in the pixels of the caller's photos.

The reference measures a model by this regression (scripts/test.py:48-65: Ridge(alpha=0) from the K landmarks to the annotated
points, fitted on a training split, then the inter-ocular error on the test split) and throws the regressor away.  Here it is an
object that can be saved next to the checkpoint and applied to new photos:

    reg = LandmarkRegressor.fit(train_tensors, [S, S], bias)     # the fit of eval_imm.regress_landmarks, coef / intercept kept
    reg.save('mafl_regressor.npz');  reg = LandmarkRegressor.load('mafl_regressor.npz', detector=det)
    kp = det.keypoints(photos, reg, boxes=[(0, y0, x0, y1, x1), ...])    # [n, M, 2] (y, x) source pixels (imm_amd/inference.py)

On the GPU the regression is an epilogue of the detector's pose head (imm_pose_head_fwd with an imm_keypoint_desc): from mu,
x = (mu + 1) / 2 * S flattened (y0, x0, y1, x1, ...) as convert_landmarks does, kp = x W + b, and the S x S frame is mapped back to
source pixels by the box's geometry (y0, x0, sy, sx): (y0 + kp_y * sy, x0 + kp_x * sx) with sy = box height / S, the inverse of
ImagePairDataset._resize_points (ratio new / old).  A box is cut from its photo with zero padding where it leaves the photo
(ImagePairDataset._crop_to_box(pad=True)) and resized to S x S on the GPU (imm_resize_crop_u8 box mode).

Host helpers here: check_boxes (validation, before anything reaches the kernels), box_geometry / image_geometry, to_source_pixels
(the epilogue's last step restated), square_box (ImagePairDataset._fit_bbox to a square)."""
import numpy as np

from .eval.eval_imm import convert_landmarks
from .ops import MAX_KEYPOINTS

MAFL_LABELS = ('left_eye', 'right_eye', 'nose', 'left_mouth', 'right_mouth')
FORMAT = 'imm-landmark-regressor-1'


class LandmarkRegressor(object):
    """A linear map from K landmarks to M annotated points: points = convert_landmarks(mu) . coef^T + intercept (the S x S frame).
    coef f64 [2M, 2K] and intercept f64 [2M] as scikit-learn's Ridge stores them (intercept zeros without bias)."""

    def __init__(self, coef, intercept, n_landmarks, image_size, bias, labels=None, dataset='', checkpoint=''):
        coef = np.asarray(coef, dtype=np.float64)
        K = int(n_landmarks)
        if coef.ndim != 2 or coef.shape[1] != 2 * K or coef.shape[0] % 2:
            raise ValueError('coef must be [2M, 2K] with K = %d, got %s' % (K, coef.shape))
        M = coef.shape[0] // 2
        intercept = np.broadcast_to(np.asarray(intercept, dtype=np.float64), (2 * M,)).copy()
        if labels is None:
            labels = MAFL_LABELS if M == len(MAFL_LABELS) else tuple('point_%d' % i for i in range(M))
        if len(labels) != M:
            raise ValueError('%d labels for %d points' % (len(labels), M))
        self.coef, self.intercept = coef, intercept
        self.K, self.M, self.S, self.bias = K, M, int(image_size), bool(bias)
        self.labels, self.dataset, self.checkpoint = tuple(str(l) for l in labels), str(dataset), str(checkpoint)

    @classmethod
    def fit(cls, train_tensors, im_size, bias=False, labels=None, dataset='', checkpoint=''):
        """train_tensors: {'gauss_yx': [N, K, 2] in [-1, 1], 'future_landmarks': [N, M, 2] pixels}; im_size: [S, S] (or S).  The fit of
        eval_imm.regress_landmarks: Ridge(alpha=0, fit_intercept=bias) on convert_landmarks."""
        import sklearn.linear_model
        size = [int(im_size), int(im_size)] if np.isscalar(im_size) else list(im_size)
        if len(size) != 2 or size[0] != size[1]:
            raise ValueError('im_size must be square, got %s' % (size,))
        x, y = convert_landmarks(train_tensors, size)
        regr = sklearn.linear_model.Ridge(alpha=0.0, fit_intercept=bias)
        regr.fit(x, y)
        K = np.asarray(train_tensors['gauss_yx']).shape[1]
        return cls(regr.coef_, regr.intercept_, K, size[0], bias, labels, dataset, checkpoint)

    def predict(self, mu):
        """mu [N, K, 2] (y, x) in [-1, 1] -> the annotated points [N, M, 2] (y, x), f64, in the S x S frame (host; the arithmetic of
        Ridge.predict on convert_landmarks)."""
        mu = np.asarray(mu)
        if mu.ndim != 3 or mu.shape[1:] != (self.K, 2):
            raise ValueError('mu must be [N, %d, 2], got %s' % (self.K, mu.shape))
        x, _ = convert_landmarks({'gauss_yx': mu, 'future_landmarks': np.zeros((mu.shape[0], 0, 2))}, [self.S, self.S])
        return (x @ self.coef.T + self.intercept).reshape(mu.shape[0], self.M, 2)

    def epilogue_weights(self):
        """(W f32 [2K, 2M], b f32 [2M]) of the pose head's keypoint epilogue; ValueError beyond its M <= 16."""
        if self.M > MAX_KEYPOINTS:
            raise ValueError('the keypoint epilogue serves at most %d annotated points, this regressor has %d' % (MAX_KEYPOINTS, self.M))
        return np.ascontiguousarray(self.coef.T, dtype=np.float32), self.intercept.astype(np.float32)

    def check(self, n_landmarks, image_size):
        if self.K != int(n_landmarks) or self.S != int(image_size):
            raise ValueError('regressor fitted for K = %d landmarks at S = %d, the detector has K = %d, S = %d' % (
                self.K, self.S, int(n_landmarks), int(image_size)))

    def save(self, path):
        with open(path, 'wb') as f:
            np.savez(f, format=np.array(FORMAT), coef=self.coef, intercept=self.intercept, K=np.int64(self.K),
                     M=np.int64(self.M), S=np.int64(self.S), bias=np.bool_(self.bias), labels=np.array(self.labels, dtype=str),
                     dataset=np.array(self.dataset), checkpoint=np.array(self.checkpoint))

    @classmethod
    def load(cls, path, detector=None):
        """A saved regressor; with `detector`, ValueError unless its K and S are the detector's."""
        with np.load(path, allow_pickle=False) as d:
            if 'format' not in d or str(d['format']) != FORMAT:
                raise ValueError('%s is not a landmark regressor file' % path)
            reg = cls(d['coef'], d['intercept'], int(d['K']), int(d['S']), bool(d['bias']), [str(l) for l in d['labels']],
                      str(d['dataset']), str(d['checkpoint']))
            if reg.M != int(d['M']):
                raise ValueError('%s: M = %d but coef has %d points' % (path, int(d['M']), reg.M))
        if detector is not None:
            reg.check(detector.K, detector.S)
        return reg


def check_boxes(boxes, n_images):
    """boxes: rows (image, y0, x0, y1, x1), or one (y0, x0, y1, x1) per image (len(boxes) == n_images), half-open, in source pixels,
    possibly reaching outside the image; values are truncated to int like ImagePairDataset._crop_to_box.  Returns int32 [n, 5];
    ValueError for an empty list, y1 <= y0, x1 <= x0 or an image index outside [0, n_images)."""
    rows = [list(b) for b in boxes]
    if not rows:
        raise ValueError('no boxes')
    if all(len(r) == 4 for r in rows):
        if len(rows) != n_images:
            raise ValueError('%d four-value boxes for %d images: give one per image, or (image, y0, x0, y1, x1) rows' % (
                len(rows), n_images))
        rows = [[i] + r for i, r in enumerate(rows)]
    if any(len(r) != 5 for r in rows):
        raise ValueError('a box is (image, y0, x0, y1, x1) or (y0, x0, y1, x1)')
    out = np.array([[int(v) for v in r] for r in rows], dtype=np.int64)
    bad = np.nonzero((out[:, 0] < 0) | (out[:, 0] >= n_images))[0]
    if bad.size:
        raise ValueError('box %d names image %d of %d' % (bad[0], out[bad[0], 0], n_images))
    bad = np.nonzero((out[:, 3] <= out[:, 1]) | (out[:, 4] <= out[:, 2]))[0]
    if bad.size:
        raise ValueError('box %d is empty: (y0, x0, y1, x1) = %s' % (bad[0], tuple(out[bad[0], 1:])))
    if np.abs(out[:, 1:]).max() >= 1 << 24:
        raise ValueError('box coordinates must stay below 2^24')
    return out.astype(np.int32)


def box_geometry(boxes, S):
    """int [n, 5] rows (image, y0, x0, y1, x1) -> f32 [n, 4] (y0, x0, sy, sx), sy = box height / S: S x S frame -> source pixels."""
    b = np.asarray(boxes, dtype=np.int64)
    S = np.float32(S)
    return np.stack([b[:, 1].astype(np.float32), b[:, 2].astype(np.float32), (b[:, 3] - b[:, 1]).astype(np.float32) / S,
                     (b[:, 4] - b[:, 2]).astype(np.float32) / S], axis=1).astype(np.float32)


def image_geometry(hw, S):
    """Whole images of sizes hw [n, 2] resized to S x S: f32 [n, 4] (0, 0, h / S, w / S)."""
    hw = np.asarray(hw, dtype=np.int64).reshape(-1, 2)
    return box_geometry(np.concatenate([np.zeros((len(hw), 3), np.int64), hw], axis=1), S)


def to_source_pixels(points, geom):
    """points [n, M, 2] (y, x) in the S x S frame, geom [n, 4] (y0, x0, sy, sx) -> source pixels (y0 + y sy, x0 + x sx), f64."""
    p = np.asarray(points, dtype=np.float64)
    g = np.asarray(geom, dtype=np.float64)
    return g[:, None, :2] + p * g[:, None, 2:]


def square_box(box, image_sz=(1, 1)):
    """(y0, x0, y1, x1) grown on one side to the aspect ratio of image_sz (a square by default), centre kept: ImagePairDataset._fit_bbox
    (f32, int32 truncation)."""
    from .datasets.impair_dataset import ImagePairDataset
    return ImagePairDataset._fit_bbox(None, box, image_sz)
