"""The rule of imm_warp_fit / imm_warp_u8 (include/imm_warp.h) restated in numpy: fit_f64, the per-row system solved in float64 by
numpy (LAPACK, partial pivoting); warp_f64, the warp in float64 written from the formulas; warp_f32, the warp in float32 in the
kernel's operation order (numpy rounds every f32 operation separately, as the kernel's unfused arithmetic does; only its log is
another implementation than the device's).  Both warps sample the ORIGINAL photos, apply the rows in row order and round to u8 after
every row.  Also the shared inputs of the kernel tests (tests/test_warp_cpu.py, tests/test_warp_gpu.py); the packing of the photos is
compose_reference's, the cap unalign_reference.within_cap."""
import numpy as np

from alignment_reference import smooth_photo


def anchors(m):
    """f64 [4 m, 2]: m points per side of [-1, 1]^2, 2 / m apart, corners included: top, right, bottom, left, walking round once."""
    pts = []
    for side in range(4):
        for i in range(m):
            t = -1.0 + 2.0 * i / m
            pts.append([(-1.0, t), (t, 1.0), (1.0, -t), (-t, -1.0)][side])
    return np.array(pts, dtype=np.float64).reshape(4 * m, 2)


def control(poses, m):
    """poses [n, K, 2] -> ctrl f32 [n, K + 4 m, 2]."""
    p = np.asarray(poses, dtype=np.float32)
    a = anchors(m).astype(np.float32)
    return np.concatenate([p, np.broadcast_to(a, (len(p),) + a.shape)], axis=1)


def U(d2):
    d2 = np.asarray(d2, dtype=np.float64)
    out = np.zeros_like(d2)
    pos = d2 > 0
    out[pos] = d2[pos] * np.log(d2[pos])
    return out


def system(ctrl, lam):
    c = np.asarray(ctrl, dtype=np.float64)
    M = len(c)
    A = np.zeros((M + 3, M + 3))
    for i in range(M):
        for j in range(M):
            dy, dx = c[i, 0] - c[j, 0], c[i, 1] - c[j, 1]
            A[i, j] = U(dy * dy + dx * dx) + (lam if i == j else 0.0)
        A[i, M], A[i, M + 1], A[i, M + 2] = 1.0, c[i, 0], c[i, 1]
        A[M, i], A[M + 1, i], A[M + 2, i] = 1.0, c[i, 0], c[i, 1]
    return A


def fit_f64(poses, mu, m, strength, lam):
    """(coef f64 [n, M + 3, 2], ctrl f32 [n, M, 2], flags int [n], cond [n]): the displacement spline of every row, its values
    strength * (mu - poses) at the landmarks and 0 at the anchors; NaN rows (flag 1) for a non-finite input or a singular system."""
    ctrl = control(poses, m)
    mu = np.asarray(mu, dtype=np.float32)
    n, K, M = len(ctrl), mu.shape[1], ctrl.shape[1]
    coef, flags, cond = np.full((n, M + 3, 2), np.nan), np.ones(n, dtype=np.int32), np.full(n, np.inf)
    for b in range(n):
        if not (np.isfinite(ctrl[b]).all() and np.isfinite(mu[b]).all()):
            continue
        A = system(ctrl[b], lam)
        rhs = np.zeros((M + 3, 2))
        rhs[:K] = strength * (mu[b].astype(np.float64) - ctrl[b, :K].astype(np.float64))
        cond[b] = np.linalg.cond(A)
        try:
            x = np.linalg.solve(A, rhs)
        except np.linalg.LinAlgError:
            continue
        if np.isfinite(x).all() and cond[b] < 1e15:
            coef[b], flags[b] = x, 0
    return coef, ctrl, flags, cond


def _box_pixels(row, h, w):
    _img, y0, x0, y1, x1 = row
    r, c = np.arange(max(y0, 0), min(y1, h)), np.arange(max(x0, 0), min(x1, w))
    if not len(r) or not len(c):
        return None
    rr, cc = np.meshgrid(r, c, indexing='ij')
    return rr.reshape(-1), cc.reshape(-1)


def warp_f64(photos, rows, ctrl, coef, inv_ramp):
    """photos: list of u8 [h, w, 3]; rows int [n, 5]; ctrl [n, M, 2], coef [n, M + 3, 2] (the values given, widened); inv_ramp
    [n, 2] -> (new photos, per photo a bool [h, w] of the pixels some row WROTE: inside a box of a row with a finite map).  Float64,
    from the formulas: q = 2 (r - y0) / H - 1, D(q), s = (r, c) + (H / 2, W / 2) D, weights (1 - t), t on the taps, (1 - a) p + a g."""
    out = [np.array(p, dtype=np.uint8, copy=True) for p in photos]
    covered = [np.zeros(p.shape[:2], dtype=bool) for p in photos]
    ctrl, coef, inv_ramp = (np.asarray(a, dtype=np.float64) for a in (ctrl, coef, inv_ramp))
    M = ctrl.shape[1]
    for b, row in enumerate(np.asarray(rows).tolist()):
        img, y0, x0, y1, x1 = row
        if img < 0 or img >= len(out):
            continue
        src, ph = photos[img], out[img]
        h, w = ph.shape[:2]
        px = _box_pixels(row, h, w)
        if px is None:
            continue
        r, c = px
        H, W = float(y1 - y0), float(x1 - x0)
        q = np.stack([2.0 * (r - y0) / H - 1.0, 2.0 * (c - x0) / W - 1.0], axis=1)
        d = q[:, None, :] - ctrl[b][None, :, :]
        D = U((d * d).sum(axis=-1)) @ coef[b, :M] + coef[b, M] + q[:, :1] * coef[b, M + 1] + q[:, 1:] * coef[b, M + 2]
        sy, sx = r + H / 2.0 * D[:, 0], c + W / 2.0 * D[:, 1]
        ok = np.isfinite(sy) & np.isfinite(sx)
        if not ok.any():
            continue
        r, c, sy, sx = r[ok], c[ok], sy[ok], sx[ok]
        fy, fx = np.floor(sy), np.floor(sx)
        ty, tx = (sy - fy)[:, None], (sx - fx)[:, None]
        yl, yh = np.clip(fy, 0, h - 1).astype(np.int64), np.clip(fy + 1, 0, h - 1).astype(np.int64)
        xl, xh = np.clip(fx, 0, w - 1).astype(np.int64), np.clip(fx + 1, 0, w - 1).astype(np.int64)
        s = src.astype(np.float64)
        g = (1 - ty) * ((1 - tx) * s[yl, xl] + tx * s[yl, xh]) + ty * ((1 - tx) * s[yh, xl] + tx * s[yh, xh])
        wy = np.minimum(1.0, (np.minimum(r - y0, y1 - 1 - r) + 0.5) * inv_ramp[b, 0])
        wx = np.minimum(1.0, (np.minimum(c - x0, x1 - 1 - c) + 0.5) * inv_ramp[b, 1])
        a = (wy * wx)[:, None]
        p = ph[r, c].astype(np.float64)
        ph[r, c] = np.clip(np.rint((1 - a) * p + a * g), 0, 255).astype(np.uint8)
        covered[img][r, c] = True
    return out, covered


def warp_f32(photos, rows, ctrl, coef, inv_ramp):
    """The same in float32 in the kernel's operation order -> new photos."""
    f32 = np.float32
    out = [np.array(p, dtype=np.uint8, copy=True) for p in photos]
    ctrl, coef, inv_ramp = (np.asarray(a, dtype=f32) for a in (ctrl, coef, inv_ramp))
    M = ctrl.shape[1]
    for b, row in enumerate(np.asarray(rows).tolist()):
        img, y0, x0, y1, x1 = row
        if img < 0 or img >= len(out):
            continue
        src, ph = photos[img], out[img]
        h, w = ph.shape[:2]
        px = _box_pixels(row, h, w)
        if px is None:
            continue
        r, c = px
        ih, iw = y1 - y0, x1 - x0
        ry, rx = f32(2.0 / np.float64(ih)), f32(2.0 / np.float64(iw))
        hy, hx = f32(0.5) * f32(ih), f32(0.5) * f32(iw)
        qy, qx = (r - y0).astype(f32) * ry - f32(1), (c - x0).astype(f32) * rx - f32(1)
        Dy, Dx = np.zeros(len(r), dtype=f32), np.zeros(len(r), dtype=f32)
        with np.errstate(all='ignore'):
            for j in range(M):
                dy, dx = qy - ctrl[b, j, 0], qx - ctrl[b, j, 1]
                d2 = dy * dy + dx * dx
                u = np.where(d2 > 0, d2 * np.log(np.where(d2 > 0, d2, f32(1))), f32(0)).astype(f32)
                Dy = Dy + coef[b, j, 0] * u
                Dx = Dx + coef[b, j, 1] * u
            Dy = ((Dy + coef[b, M, 0]) + coef[b, M + 1, 0] * qy) + coef[b, M + 2, 0] * qx
            Dx = ((Dx + coef[b, M, 1]) + coef[b, M + 1, 1] * qy) + coef[b, M + 2, 1] * qx
            sy, sx = r.astype(f32) + hy * Dy, c.astype(f32) + hx * Dx
        assert sy.dtype == f32 and sx.dtype == f32
        ok = np.isfinite(sy) & np.isfinite(sx)
        if not ok.any():
            continue
        r, c, sy, sx = r[ok], c[ok], sy[ok], sx[ok]
        fy, fx = np.floor(sy), np.floor(sx)
        ty, tx = (sy - fy)[:, None], (sx - fx)[:, None]
        iy = np.minimum(np.maximum(fy, f32(-1)), f32(h)).astype(np.int64)
        ix = np.minimum(np.maximum(fx, f32(-1)), f32(w)).astype(np.int64)
        yl, yh = np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
        xl, xh = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1)
        s = src.astype(f32)
        tl, tr, bl, br = s[yl, xl], s[yl, xh], s[yh, xl], s[yh, xh]
        top = tl + (tr - tl) * tx
        bot = bl + (br - bl) * tx
        g = top + (bot - top) * ty
        wy = np.minimum(f32(1), (np.minimum(r - y0, y1 - 1 - r).astype(f32) + f32(0.5)) * inv_ramp[b, 0])
        wx = np.minimum(f32(1), (np.minimum(c - x0, x1 - 1 - c).astype(f32) + f32(0.5)) * inv_ramp[b, 1])
        a = (wy * wx)[:, None]
        p = ph[r, c].astype(f32)
        d = g - p
        mm = a * d
        v = np.minimum(np.maximum(np.rint(p + mm), f32(0)), f32(255))
        assert v.dtype == f32
        ph[r, c] = v.astype(np.uint8)
    return out


def inv_ramp(rows, feather):
    """imm_compose_u8's reciprocal ramp widths, f32 [n, 2]: 1 / (feather * side), 2 where feather * side <= 0.5."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 5)
    ramp = float(feather) * (rows[:, 3:5] - rows[:, 1:3]).astype(np.float64)
    return np.where(ramp <= 0.5, 2.0, 1.0 / np.maximum(ramp, 0.5)).astype(np.float32)


def no_band(photos):
    """within_cap's border band for a warp: empty (a warp's coverage is the integer box, the same in f32 and f64)."""
    return [np.zeros(p.shape[:2], dtype=bool) for p in photos]


# ---- the kernel case: every way a box can meet a photo -------------------------------------------------------------------------------
# Photos 0..2 are 23 x 37, 40 x 40 and 9 x 64 (odd widths: photo rows start at any byte); photo 3 has no row.  Box sides run from 1 to
# 40 px.  Rows 2, 6 and 10 overlap each other on photo 1 and are given out of spatial order, with rows of other photos between them; the
# 40 x 31 box (row 4) lies under all three.
KERNEL_PHOTOS = [(23, 37), (40, 40), (9, 64), (7, 5)]
KERNEL_ROWS = [
    (0, 3, 5, 19, 21),        # 0   16 x 16; poses == mu: the identity row
    (2, 4, 20, 5, 29),        # 1   1 x 9: H == 1
    (1, 18, 2, 36, 26),       # 2   overlap C
    (0, -6, 24, 8, 36),       # 3   over the top edge
    (1, 0, 4, 40, 35),        # 4   40 x 31
    (2, 2, 50, 7, 57),        # 5   5 x 7; a NaN landmark: flagged, writes nothing
    (1, 10, 10, 30, 30),      # 6   overlap A
    (2, 0, 40, 9, 41),        # 7   9 x 1: W == 1
    (0, 18, 0, 30, 9),        # 8   over the bottom and the left edge
    (1, 50, 50, 70, 80),      # 9   wholly outside
    (1, 5, 20, 25, 38),       # 10  overlap B
    (2, 1, -5, 8, 6),         # 11  over the left edge
    (2, 3, 58, 12, 70),       # 12  over the right and the bottom edge
    (7, 2, 2, 12, 12),        # 13  an image index past the last photo
    (-1, 2, 2, 12, 12),       # 14  a negative image index
]
OVERLAPPING = (2, 6, 10)
IDENTITY_ROW, NAN_ROW, OUTSIDE_ROW, BAD_IMAGE_ROWS = 0, 5, 9, (13, 14)
# (K, anchors per side): M = 3, 18 and 80 control points
KERNEL_SHAPES = [(3, 0), (10, 2), (64, 4)]
LAMS = (0.0, 1e-2)
FEATHERS = (0.0, 0.125, 0.5)
NOISE_SIGMA = 0.05
# Seed for which warp_f32 stays at or below half the cap's share against warp_f64 for every shape, lam and feather of the tests:
# checked on the CPU by test_warp_cpu.test_f32_restatement_against_f64
KERNEL_SEED = 7


def landmarks(K, n, rng, sigma=NOISE_SIGMA):
    """(mu, poses) f32 [n, K, 2]: the poses (the spline's control points) on a jittered grid over [-0.8, 0.8]^2 (cells of side
    1.6 / ceil(sqrt(K)), jitter a quarter cell either way, a random choice of K cells), so that no two lie close and the systems stay
    well conditioned; mu = poses + N(0, sigma)."""
    g = int(np.ceil(np.sqrt(K)))
    cell = 1.6 / g
    poses = np.zeros((n, K, 2))
    for b in range(n):
        pick = rng.permutation(g * g)[:K]
        centre = np.stack([pick // g, pick % g], axis=1) * cell - 0.8 + cell / 2
        poses[b] = centre + rng.uniform(-cell / 4, cell / 4, size=(K, 2))
    mu = poses + rng.normal(0.0, sigma, size=poses.shape)
    return mu.astype(np.float32), poses.astype(np.float32)


def kernel_photos(K, seed):
    """Uniform-noise photos for K <= 10; smooth, low-pass photos for more landmarks, whose f32 sums are longer (photo 3 always grey
    noise)."""
    rng = np.random.RandomState(seed + 1000)
    if K <= 10:
        photos = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in KERNEL_PHOTOS]
    else:
        photos = [smooth_photo(h, w, seed + i) for i, (h, w) in enumerate(KERNEL_PHOTOS)]
    photos[3] = np.repeat(rng.randint(0, 256, size=KERNEL_PHOTOS[3] + (1,)).astype(np.uint8), 3, axis=2)
    return photos


def kernel_case(K, m, seed=KERNEL_SEED):
    """(photos, rows int32 [n, 5], mu f32 [n, K, 2], poses f32 [n, K, 2])."""
    rng = np.random.RandomState(seed + 31 * K)
    rows = np.array(KERNEL_ROWS, dtype=np.int32)
    mu, poses = landmarks(K, len(rows), rng)
    mu[IDENTITY_ROW] = poses[IDENTITY_ROW]
    mu[NAN_ROW, K // 2, 1] = np.nan
    return kernel_photos(K, seed), rows, mu, poses


def shifted(photo, row, dy, dx):
    """The photo with the box of `row` replaced by the photo's pixels at (r - dy, c - dx), edge-clamped."""
    h, w = photo.shape[:2]
    _img, y0, x0, y1, x1 = [int(v) for v in row]
    out = photo.copy()
    r, c = np.arange(max(y0, 0), min(y1, h)), np.arange(max(x0, 0), min(x1, w))
    out[r[0]:r[-1] + 1, c[0]:c[-1] + 1] = photo[np.clip(r - dy, 0, h - 1)][:, np.clip(c - dx, 0, w - 1)]
    return out


def hw_of(photos):
    return np.array([p.shape[:2] for p in photos], dtype=np.int32)
