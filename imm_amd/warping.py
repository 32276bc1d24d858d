"""Faces re-posed from their own pixels: the host side of LandmarkDetector.warp (include/imm_warp.h states the rule).

repose() and reenact() change a face through the generator: a 300-pixel face comes back as an up-sampled 128-pixel render.  warp()
moves the photo's OWN pixels instead.  Per face, a thin-plate spline is fitted whose control points are the face's target landmarks
(the pose) and a ring of anchors on the border of the box frame; it carries every target landmark back to the face's own landmark
and every anchor to itself, so the face takes the pose while the box border stays where it is and the result blends into the photo.
The spline is stored as a DISPLACEMENT (its values are strength * (mu - pose) at the landmarks and 0 at the anchors): poses equal to
the face's own landmarks give exactly zero coefficients, and the photo comes back bit for bit.

Here: the anchors, the control points, the f64 fit (the arithmetic imm_warp_fit stands for: the same system, eliminated in the
same order), the argument checks of warp() and PhotoWarp, what warp(return_transform=True) returns.  Nothing here needs a GPU."""
import numpy as np

MAX_POINTS = 80                # control points of one spline (landmarks + anchors): imm_warp_fit's matrix lives in LDS
MIN_DISTANCE = 1e-6            # control points of a row closer than this are refused when the poses are known on the host


def warp_anchors(m):
    """f64 [4 m, 2] (y, x): m points per side of [-1, 1]^2, equally spaced (2 / m apart), corners included, from (-1, -1) along the top
    side (y = -1), then the right (x = 1), the bottom (y = 1, right to left) and the left one (bottom to top).  m = 2: the corners and
    the edge midpoints.  m = 0: no anchors, [0, 2]."""
    if int(m) != m or m < 0:
        raise ValueError('anchors must be an integer >= 0 (points per side of the box frame), got %r' % (m,))
    m = int(m)
    t = -1.0 + 2.0 * np.arange(m, dtype=np.float64) / max(m, 1)
    one = np.ones(m)
    top = np.stack([-one, t], axis=1)
    right = np.stack([t, one], axis=1)
    bottom = np.stack([one, -t], axis=1)
    left = np.stack([-t, -one], axis=1)
    return np.concatenate([top, right, bottom, left], axis=0).reshape(4 * m, 2)


def control_points(poses, m):
    """poses [n, K, 2] -> f32 [n, K + 4 m, 2]: each row's target landmarks followed by the anchors (rounded to f32, as the device
    holds them)."""
    p = np.asarray(poses, dtype=np.float32)
    if p.ndim != 3 or p.shape[2] != 2:
        raise ValueError('poses must be [n, K, 2], got %s' % (p.shape,))
    a = warp_anchors(m).astype(np.float32)
    return np.concatenate([p, np.broadcast_to(a, (p.shape[0],) + a.shape)], axis=1)


def check_points(K, m):
    """M = K + 4 m, refused outside [3, MAX_POINTS]."""
    M = int(K) + 4 * int(m)
    if M < 3:
        raise ValueError('a warp needs M = K + 4 * anchors >= 3 control points (an affine part has three unknowns per axis), got %d' % M)
    if M > MAX_POINTS:
        raise ValueError('a warp serves M = K + 4 * anchors <= %d control points, got %d + 4 * %d = %d' % (MAX_POINTS, K, m, M))
    return M


def tps_u(d2):
    """U(d2) = d2 log d2, U(0) = 0."""
    d2 = np.asarray(d2, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(d2 > 0.0, d2 * np.log(np.where(d2 > 0.0, d2, 1.0)), 0.0)


def system_matrix(ctrl, lam):
    """The (M + 3) x (M + 3) matrix of one row: [[U + lam I, 1, ctrl], [1^T, 0, 0], [ctrl^T, 0, 0]], f64, from ctrl [M, 2]."""
    c = np.asarray(ctrl, dtype=np.float64)
    M = len(c)
    d = c[:, None, :] - c[None, :, :]
    A = np.zeros((M + 3, M + 3))
    A[:M, :M] = tps_u(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + float(lam) * np.eye(M)
    A[:M, M] = 1.0
    A[:M, M + 1:] = c
    A[M, :M] = 1.0
    A[M + 1:, :M] = c.T
    return A


def solve_pivoting(A, rhs):
    """x with A x = rhs by Gaussian elimination with partial pivoting, in imm_warp_fit's order: per column the row of the largest
    |value| (the first of equals) becomes the pivot row, the multipliers of the column are formed by one division each, the trailing
    block and the right-hand sides lose multiplier * pivot row; then a column-oriented back substitution.  Every operation is rounded
    separately.  None when a pivot is zero or not finite (numpy's solver would divide by a pivot of rounding noise instead)."""
    a = np.concatenate([np.asarray(A, dtype=np.float64), np.asarray(rhs, dtype=np.float64)], axis=1)
    N = a.shape[0]
    with np.errstate(all='ignore'):
        for k in range(N):
            piv = k + int(np.argmax(np.abs(a[k:, k])))
            pv = a[piv, k]
            if not np.isfinite(pv) or pv == 0.0:
                return None
            if piv != k:
                a[[k, piv], k:] = a[[piv, k], k:]
            a[k + 1:, k] = a[k + 1:, k] / pv
            a[k + 1:, k + 1:] = a[k + 1:, k + 1:] - a[k + 1:, k:k + 1] * a[k:k + 1, k + 1:]
        for k in range(N - 1, -1, -1):
            a[k, N:] = a[k, N:] / a[k, k]
            a[:k, N:] = a[:k, N:] - a[:k, k:k + 1] * a[k:k + 1, N:]
    return a[:, N:]


def fit_warp(poses, mu, m, strength=1.0, lam=0.0):
    """The f64 host fit: poses, mu [n, K, 2] (read as f32, as the device holds them) -> (coef f64 [n, M + 3, 2], ctrl f32 [n, M, 2],
    flags int32 [n]).  Row b solves system_matrix(ctrl_b, lam) . [w; a] = [strength * (mu_b - poses_b); 0] by solve_pivoting.  A row
    with a non-finite input, or with a pivot that is zero or not finite, gets NaN coefficients and flag 1."""
    ctrl = control_points(poses, m)
    mu = np.asarray(mu, dtype=np.float32)
    n, K = mu.shape[0], mu.shape[1]
    if ctrl.shape[0] != n or ctrl.shape[1] != K + 4 * int(m):
        raise ValueError('poses %s and mu %s differ in shape' % (np.shape(poses), mu.shape))
    M = check_points(K, m)
    coef = np.full((n, M + 3, 2), np.nan)
    flags = np.ones(n, dtype=np.int32)
    for b in range(n):
        if not (np.isfinite(ctrl[b]).all() and np.isfinite(mu[b]).all()):
            continue
        rhs = np.zeros((M + 3, 2))
        rhs[:K] = float(strength) * (mu[b].astype(np.float64) - ctrl[b, :K].astype(np.float64))
        x = solve_pivoting(system_matrix(ctrl[b], lam), rhs)
        if x is not None:
            coef[b], flags[b] = x, 0
    return coef, ctrl, flags


def displacement(coef, ctrl, q):
    """D(q) f64 [P, 2] of one row at frame points q [P, 2]: sum_j w_j U(|q - ctrl_j|^2) + a_0 + a_1 q_y + a_2 q_x."""
    coef, c, q = np.asarray(coef, dtype=np.float64), np.asarray(ctrl, dtype=np.float64), np.asarray(q, dtype=np.float64)
    M = len(c)
    d = q[:, None, :] - c[None, :, :]
    u = tps_u(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
    return u @ coef[:M] + coef[M] + q[:, :1] * coef[M + 1] + q[:, 1:] * coef[M + 2]


def check_spline(anchors, lam, strength, K):
    """warp()'s anchors, lam and strength checked: (m, lam, strength, M)."""
    m = warp_anchors(anchors).shape[0] // 4
    lam, strength = float(lam), float(strength)
    if not (lam >= 0.0 and np.isfinite(lam)):
        raise ValueError('lam must be finite and >= 0, got %r' % (lam,))
    if not np.isfinite(strength):
        raise ValueError('strength must be finite, got %r' % (strength,))
    return m, lam, strength, check_points(K, m)


def plan_warp(photos, poses, boxes, pose_boxes, feather, K, anchors=2, lam=0.0, strength=1.0):
    """warp()'s arguments checked on the host, before anything reaches the device: (photos as decoded u8 arrays, box rows int32 [n, 5],
    poses, feather, m, lam, strength, M), photos / poses / boxes / pose_boxes in generation.plan_repose's forms and poses as it returns
    them.  Poses given as host landmarks are known here (a device tensor stays where it is): a row whose control points (target landmarks and anchors) are not finite or lie
    closer than MIN_DISTANCE to each other is refused (its system would be singular, or as good as)."""
    from .generation import plan_repose
    m, lam, strength, M = check_spline(anchors, lam, strength, K)
    photos, rows, pose, feather = plan_repose(photos, poses, boxes, pose_boxes, feather, K)
    if pose[0] == 'landmarks' and not pose[1].is_cuda:          # a device tensor is not read back: its rows are judged by the fit
        ctrl = control_points(pose[1].numpy(), m).astype(np.float64)
        if not np.isfinite(ctrl).all():
            raise ValueError('poses must be finite')
        d = ctrl[:, :, None, :] - ctrl[:, None, :, :]
        d2 = (d * d).sum(axis=-1) + np.eye(M) * 4.0
        if d2.min() < MIN_DISTANCE * MIN_DISTANCE:
            b, i, j = np.unravel_index(int(np.argmin(d2)), d2.shape)
            raise ValueError('pose %d: control points %d and %d (landmarks 0..%d, then the anchors) lie closer than %g' % (
                b, i, j, K - 1, MIN_DISTANCE))
    return photos, rows, pose, feather, m, lam, strength, M


class PhotoWarp(object):
    """What warp(return_transform=True) returns: the splines of the call's rows.  coef f32 [n, M + 3, 2] and ctrl f32 [n, M, 2] (device
    tensors, as imm_warp_fit wrote them), rows int32 [n, 5] (host), mu f32 [n, K, 2] (the faces' own landmarks), poses f32 [n, K, 2],
    flags int32 [n] (bit 0: the row had no usable fit and its box was left alone), and the call's strength, lam and anchors."""

    def __init__(self, coef, ctrl, rows, mu, poses, flags, strength, lam, anchors):
        self.coef, self.ctrl, self.rows, self.mu, self.poses, self.flags = coef, ctrl, np.asarray(rows, dtype=np.int32), mu, poses, flags
        self.strength, self.lam, self.anchors = float(strength), float(lam), int(anchors)

    def to_source(self, points_px):
        """points_px [n, P, 2]: (y, x) photo pixels of the RESULT, row b's in the photo of row b -> f64 [n, P, 2], the photo pixels of
        the ORIGINAL the warp took them from (the kernel's map s, in f64 from the f32 coefficients; blending and clamping apart)."""
        pts = np.asarray(points_px, dtype=np.float64)
        n = len(self.rows)
        if pts.ndim != 3 or pts.shape[0] != n or pts.shape[2] != 2:
            raise ValueError('points_px must be [%d, P, 2], got %s' % (n, pts.shape))
        coef, ctrl = _host(self.coef), _host(self.ctrl)
        org = self.rows[:, 1:3].astype(np.float64)
        half = (self.rows[:, 3:5] - self.rows[:, 1:3]).astype(np.float64) / 2.0
        out = np.empty_like(pts)
        for b in range(n):
            q = (pts[b] - org[b]) / half[b] - 1.0
            out[b] = pts[b] + half[b] * displacement(coef[b], ctrl[b], q)
        return out


def _host(t):
    return t.detach().cpu().numpy() if hasattr(t, 'detach') else np.asarray(t)
