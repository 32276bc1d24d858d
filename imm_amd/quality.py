"""Landmark quality: two scores per face that say how far its landmarks deserve trust, and a gate that applies thresholds to them.

The soft-argmax always returns finite landmarks, on a face and on a wall alike.  After every pose program the detector's buffers hold
what tells the two apart, and one small kernel (include/imm_score.h states the rule once) turns it into

    sbar        the mean over the K landmarks of how widely each one's probability is spread about its mean (in units of the [-1, 1]
                landmark frame: 0 for a one-hot heat map, about 0.87 for a uniform 16 x 16 one)
    residual    the share of the landmarks' scatter that the best similarity of a reference shape leaves unexplained, in [0, 1]
                (a LandmarkTemplate for stills; the first frame's own shape in the tracker)

    q = det.quality(photos, boxes, template=tpl)         # a LandmarkQuality: q.sbar, q.residual, q.spread, q.mu, q.py, q.px
    gate = QualityGate.fit(q, quantile=0.99, margin=1.5) # thresholds from faces KNOWN to be good
    tr = det.tracker(gate=gate).track(frames, boxes)     # a face that fails the gate on a frame is lost on that frame: tr.unsure

NOTHING HERE IS MEASURED ON FOOTAGE.  Whether the spread or the residual separates faces from non-faces, and at what thresholds, is not
known: there is no trained checkpoint and no video where this was written.  So no default threshold is shipped: QualityGate() applies
none, QualityGate.fit has no default for its quantile or its margin, and a caller who wants a gate fits one on faces of their own.

This module holds the host side and imports without a GPU."""
import math

import numpy as np

FORMAT = 'imm-quality-gate-1'
FLAG_SPREAD, FLAG_RESIDUAL = 1, 2


def _threshold(value, name):
    if value is None:
        return None
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError('%s must be a finite number > 0 or None, got %r' % (name, value))
    if not (math.isfinite(v) and v > 0):
        raise ValueError('%s must be finite and > 0 (None: not applied), got %r' % (name, value))
    return v


def _host(t):
    """A score array on the host as f64 (a device tensor comes through ops.download)."""
    if hasattr(t, 'is_cuda'):
        if t.is_cuda:
            from . import ops
            t = ops.download(t.contiguous())
        t = t.detach().numpy()
    return np.asarray(t, dtype=np.float64)


class QualityGate(object):
    """Thresholds on the two scores: a face whose mean spread exceeds max_spread, or whose shape residual exceeds max_residual, or whose
    score is NaN, is unsure.  None: that score is not applied (the kernel takes +inf).  There are no default thresholds: nobody has
    measured these scores on footage.  K, S and the heat-map side the thresholds were fitted at are kept when known (fit on a
    LandmarkQuality), written by save and held against a detector by check."""

    def __init__(self, max_spread=None, max_residual=None, K=None, S=None, heatmap=None):
        self.max_spread, self.max_residual = _threshold(max_spread, 'max_spread'), _threshold(max_residual, 'max_residual')
        self.K, self.S, self.heatmap = (None if v is None else int(v) for v in (K, S, heatmap))

    def __repr__(self):
        return 'QualityGate(max_spread=%r, max_residual=%r)' % (self.max_spread, self.max_residual)

    @classmethod
    def fit(cls, quality, quantile, margin):
        """Thresholds from faces known to be good: margin * np.quantile(sbar, quantile), and the same of the residual unless every
        residual is 0 (no reference was used).  quality: a LandmarkQuality, or (sbar, residual) arrays.  quantile in (0, 1] and
        margin >= 1 have no defaults: which values suit footage is unmeasured."""
        q, m = float(quantile), float(margin)
        if not (0.0 < q <= 1.0):
            raise ValueError('quantile must lie in (0, 1], got %r' % (quantile,))
        if not (math.isfinite(m) and m >= 1.0):
            raise ValueError('margin must be finite and >= 1, got %r' % (margin,))
        if isinstance(quality, LandmarkQuality):
            sbar, residual = _host(quality.sbar), _host(quality.residual)
            meta = dict(K=quality.mu.shape[1], S=quality.S, heatmap=quality.py.shape[1])
        else:
            sbar, residual = (_host(v).reshape(-1) for v in quality)
            meta = {}
        if sbar.size == 0 or sbar.shape != residual.shape:
            raise ValueError('fit needs one (sbar, residual) per face of at least one face, got %s and %s' % (sbar.shape, residual.shape))
        if not (np.isfinite(sbar).all() and np.isfinite(residual).all()):
            raise ValueError('fit needs finite scores: a NaN score marks a face that is not good')
        spread = m * float(np.quantile(sbar, q))
        resid = None if not residual.any() else m * float(np.quantile(residual, q))
        return cls(spread, resid, **meta)

    def check(self, n_landmarks, image_size):
        """ValueError when the gate was fitted at another K or S (a gate made by hand holds neither and passes)."""
        for name, mine, theirs in (('K', self.K, n_landmarks), ('S', self.S, image_size)):
            if mine is not None and mine != int(theirs):
                raise ValueError('quality gate fitted at %s = %d, the detector has %s = %d' % (name, mine, name, int(theirs)))

    def save(self, path):
        nan = lambda v: np.float64('nan') if v is None else np.float64(v)
        num = lambda v: np.int64(-1) if v is None else np.int64(v)
        with open(path, 'wb') as f:
            np.savez(f, format=np.array(FORMAT), max_spread=nan(self.max_spread), max_residual=nan(self.max_residual), K=num(self.K),
                     S=num(self.S), heatmap=num(self.heatmap))

    @classmethod
    def load(cls, path, detector=None):
        """A saved gate; with `detector`, ValueError unless its K and S are the detector's."""
        with np.load(path, allow_pickle=False) as d:
            if 'format' not in d or str(d['format']) != FORMAT:
                raise ValueError('%s is not a quality gate file' % path)
            val = lambda k: None if np.isnan(d[k]) else float(d[k])
            num = lambda k: None if int(d[k]) < 0 else int(d[k])
            gate = cls(val('max_spread'), val('max_residual'), num('K'), num('S'), num('heatmap'))
        if detector is not None:
            gate.check(detector.K, detector.S)
        return gate


def check_gate(gate, n_landmarks=None, image_size=None):
    """A `gate` argument: None or a QualityGate (ValueError otherwise), held against K and S when they are given."""
    if gate is not None and not isinstance(gate, QualityGate):
        raise ValueError('gate must be a quality.QualityGate or None, got %r' % (gate,))
    if gate is not None and n_landmarks is not None:
        gate.check(n_landmarks, image_size)
    return gate


class LandmarkQuality(object):
    """What LandmarkDetector.quality returns, n rows, tensors on the detector's device (or the host after .cpu()): mu f32 [n, K, 2] the
    landmarks (detect()'s bits), spread f32 [n, K], score f32 [n, 2] = (sbar, residual), flags int32 [n] (bit 0: the spread fails the
    gate, bit 1: the residual does; 0 without a gate unless a score is NaN) and the soft-argmax marginals py f32 [n, h, K], px f32
    [n, w, K] the scores were taken from.  S: the detector's image size."""

    def __init__(self, mu, spread, score, flags, py, px, S=None):
        self.mu, self.spread, self.score, self.flags, self.py, self.px, self.S = mu, spread, score, flags, py, px, S

    def __len__(self):
        return int(self.mu.shape[0])

    @property
    def sbar(self):
        """f32 [n]: the mean spread of the K landmarks."""
        return self.score[:, 0]

    @property
    def residual(self):
        """f32 [n]: the shape residual against the template; 0 without one."""
        return self.score[:, 1]

    @property
    def unsure(self):
        """bool [n]: a score failed the gate or is NaN."""
        return self.flags != 0

    def cpu(self):
        from . import ops
        get = lambda t: ops.download(t.contiguous())
        return LandmarkQuality(get(self.mu), get(self.spread), get(self.score), get(self.flags), get(self.py), get(self.px), self.S)
