"""The pixel rule of imm_unalign_maps / imm_unalign_u8 (include/imm_unalign.h) restated in numpy: maps_f64, the map kernel's
arithmetic in float64 in the kernel's operation order; unalign_f32, the paste in float32 in the kernel's order (numpy rounds every
f32 operation separately, as the kernel's unfused arithmetic does); unalign_f64, the paste in float64 written from the formulas, with
its own inverse.  All apply the rows in row order and round to u8 after every row.  Also the shared inputs of the kernel tests
(tests/test_unalign_cpu.py, tests/test_unalign_gpu.py); the packing of the photos is compose_reference's."""
import numpy as np

S_KERNEL = 16                       # image_size and out_size of the kernel case
BORDER_BAND = 1e-3                  # px: pixels whose f64 coordinate lies this close to the frame border are left out of f32-vs-f64


def maps_f64(coef, geom, img, hw, S, So):
    """coef f32 [n, 3, 2], geom f32 [n, 4], img int [n], hw int [n_images, 2] -> (fwd f64 [n, 6] (NaN rows for det == 0, a non-finite
    value or an image index out of range), bbox int32 [n, 4], B f64 [n, 2, 2], t f64 [n, 2]).  fwd.astype(float32) is what the kernel
    writes: the f32 inputs widened, every operation in float64 in the kernel's order, one rounding at the end."""
    coef = np.asarray(coef, dtype=np.float32).astype(np.float64).reshape(-1, 3, 2)
    geom = np.asarray(geom, dtype=np.float32).astype(np.float64).reshape(-1, 4)
    img = np.asarray(img, dtype=np.int64).reshape(-1)
    hw = np.asarray(hw, dtype=np.int64).reshape(-1, 2)
    dS, dSo = np.float64(S), np.float64(So)
    with np.errstate(all='ignore'):
        k = geom[:, 2:4] * dS                                               # [n, a]
        c0, c1, c2 = coef[:, 0, :], coef[:, 1, :], coef[:, 2, :]
        B = np.stack([(k * c1) / dSo, (k * c2) / dSo], axis=2)              # B[n, a, 0], B[n, a, 1]
        t = geom[:, 0:2] + (k * 0.5) * (((c0 + 1.0) - c1) - c2)
        det = B[:, 0, 0] * B[:, 1, 1] - B[:, 0, 1] * B[:, 1, 0]
        m00, m01, m10, m11 = B[:, 1, 1] / det, -B[:, 0, 1] / det, -B[:, 1, 0] / det, B[:, 0, 0] / det
        m02 = -(m00 * t[:, 0] + m01 * t[:, 1])
        m12 = -(m10 * t[:, 0] + m11 * t[:, 1])
        fwd = np.stack([m00, m01, m02, m10, m11, m12], axis=1)
        ok = (img >= 0) & (img < len(hw)) & (det != 0.0) & np.isfinite(fwd.astype(np.float32)).all(axis=1)
        e = dSo - 1.0
        corners = np.stack([t, B[:, :, 0] * e + t, B[:, :, 1] * e + t, (B[:, :, 0] * e + B[:, :, 1] * e) + t], axis=0)    # [4, n, a]
        ok &= np.isfinite(corners).all(axis=(0, 2))
    lo, hi = corners.min(axis=0), corners.max(axis=0)
    bbox = np.zeros((len(img), 4), dtype=np.int32)
    for b in np.nonzero(ok)[0]:
        sh, sw = hw[img[b]]
        y0, y1 = max(np.floor(lo[b, 0]) - 1.0, 0.0), min(np.ceil(hi[b, 0]) + 2.0, float(sh))
        x0, x1 = max(np.floor(lo[b, 1]) - 1.0, 0.0), min(np.ceil(hi[b, 1]) + 2.0, float(sw))
        if y1 > y0 and x1 > x0:
            bbox[b] = (int(y0), int(x0), int(y1), int(x1))
    fwd = np.where(ok[:, None], fwd, np.nan)
    return fwd, bbox, B, t


def cover_f32(hw, m, So):
    """(fi, fj, covered) f32 [h, w] of one photo of hw = (h, w) under the forward map m f32 [6], in the kernel's operation order."""
    f32 = np.float32
    m = np.asarray(m, dtype=f32)
    r, c = np.arange(hw[0], dtype=f32)[:, None], np.arange(hw[1], dtype=f32)[None, :]
    with np.errstate(invalid='ignore'):
        fi = (m[0] * r + m[1] * c) + m[2]
        fj = (m[3] * r + m[4] * c) + m[5]
        edge = f32(So - 1)
        cov = (fi >= 0) & (fi <= edge) & (fj >= 0) & (fj <= edge)             # NaN compares false: a NaN map covers nothing
    assert fi.dtype == f32 and fj.dtype == f32
    return fi, fj, cov


def unalign_f32(photos, img, fwd32, faces, inv_ramp, So, return_cover=False):
    """photos: list of u8 [h, w, 3]; img int [n]; fwd32 f32 [n, 6]; faces f32 [n, So, So, >= 3]; inv_ramp: the f32 reciprocal of the
    ramp -> new list of u8 photos (and with return_cover the per-row bool masks [h, w] of the pixels each row covers, None for a row
    without a photo)."""
    f32 = np.float32
    out = [np.array(p, dtype=np.uint8, copy=True) for p in photos]
    faces = np.asarray(faces, dtype=f32)
    fwd32 = np.asarray(fwd32, dtype=f32).reshape(-1, 6)
    inv, edge = f32(inv_ramp), f32(So - 1)
    covers = []
    for b, i in enumerate(np.asarray(img).tolist()):
        if i < 0 or i >= len(out):
            covers.append(None)
            continue
        ph = out[i]
        fi, fj, cov = cover_f32(ph.shape[:2], fwd32[b], So)
        covers.append(cov)
        if not cov.any():
            continue
        fi, fj = fi[cov], fj[cov]
        yl, xl = np.minimum(np.floor(fi).astype(np.int64), So - 1), np.minimum(np.floor(fj).astype(np.int64), So - 1)
        yh, xh = np.minimum(yl + 1, So - 1), np.minimum(xl + 1, So - 1)
        ty, tx = (fi - yl.astype(f32))[:, None], (fj - xl.astype(f32))[:, None]
        f = faces[b, :, :, :3]
        tl, tr, bl, br = f[yl, xl], f[yl, xh], f[yh, xl], f[yh, xh]
        top = tl + (tr - tl) * tx
        bot = bl + (br - bl) * tx
        g = top + (bot - top) * ty
        g = np.minimum(np.maximum(g, f32(0)), f32(255))
        wy = np.minimum(f32(1), (np.minimum(fi, edge - fi) + f32(0.5)) * inv)
        wx = np.minimum(f32(1), (np.minimum(fj, edge - fj) + f32(0.5)) * inv)
        a = (wy * wx)[:, None]
        p = ph[cov].astype(f32)
        d = g - p
        m = a * d
        v = np.rint(p + m)
        assert v.dtype == f32 and v.min() >= 0 and v.max() <= 255
        ph[cov] = v.astype(np.uint8)
    return (out, covers) if return_cover else out


def unalign_f64(photos, img, B, t, faces, inv_ramp, So, band=BORDER_BAND):
    """The same rule in float64, written from the formulas: (fi, fj) = B^-1 ((r, c) - t) with numpy's inverse, weights (1 - t), t on the
    taps, (1 - a) p + a g.  B f64 [n, 2, 2], t f64 [n, 2]: the backward maps (maps_f64 returns them).  Returns (new photos, per photo a
    bool [h, w] of the pixels at least one row covers, per photo a bool [h, w] of the pixels whose coordinate under some row lies within
    `band` px of the frame border 0 or So - 1 without lying ON it: there f32 and f64 may disagree on the coverage itself.  A coordinate
    that is exactly 0 or So - 1 in f64 (every border pixel of the integer translation row: 60 of them at So = 16) is covered in both
    restatements and stays in the comparison)."""
    out = [np.array(p, dtype=np.uint8, copy=True) for p in photos]
    covered = [np.zeros(p.shape[:2], dtype=bool) for p in photos]
    near = [np.zeros(p.shape[:2], dtype=bool) for p in photos]
    faces = np.asarray(faces, dtype=np.float64)
    inv, e = float(inv_ramp), So - 1.0
    for b, i in enumerate(np.asarray(img).tolist()):
        if i < 0 or i >= len(out) or not np.isfinite(B[b]).all() or not np.isfinite(t[b]).all() or np.linalg.det(B[b]) == 0.0:
            continue
        ph = out[i]
        h, w = ph.shape[:2]
        rc = np.stack(np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij'), axis=-1)
        f = (rc - t[b]) @ np.linalg.inv(B[b]).T
        fi, fj = f[..., 0], f[..., 1]
        cov = (fi >= 0) & (fi <= e) & (fj >= 0) & (fj <= e)
        wide = (fi >= -band) & (fi <= e + band) & (fj >= -band) & (fj <= e + band)
        di, dj = np.minimum(np.abs(fi), np.abs(fi - e)), np.minimum(np.abs(fj), np.abs(fj - e))
        near[i] |= wide & (((di < band) & (di > 0)) | ((dj < band) & (dj > 0)))
        covered[i] |= cov
        if not cov.any():
            continue
        fi, fj = fi[cov], fj[cov]
        yl, xl = np.minimum(np.floor(fi).astype(np.int64), So - 1), np.minimum(np.floor(fj).astype(np.int64), So - 1)
        yh, xh = np.minimum(yl + 1, So - 1), np.minimum(xl + 1, So - 1)
        ty, tx = (fi - yl)[:, None], (fj - xl)[:, None]
        fc = faces[b, :, :, :3]
        g = (1 - ty) * ((1 - tx) * fc[yl, xl] + tx * fc[yl, xh]) + ty * ((1 - tx) * fc[yh, xl] + tx * fc[yh, xh])
        g = np.clip(g, 0.0, 255.0)
        wy = np.minimum(1.0, (np.minimum(fi, e - fi) + 0.5) * inv)
        wx = np.minimum(1.0, (np.minimum(fj, e - fj) + 0.5) * inv)
        a = (wy * wx)[:, None]
        p = ph[cov].astype(np.float64)
        ph[cov] = np.rint((1 - a) * p + a * g).astype(np.uint8)
    return out, covered, near


def within_cap(a, b, covered, near):
    """The cap between two pastes of the same rows (lists of u8 photos): at most one grey level anywhere and at most 0.5 % of the covered
    pixels differing, the pixels of the border band left out, those being at most 0.5 % of the covered pixels themselves.
    Returns (pixels differing, largest difference, pixels left out, covered pixels) after asserting the cap."""
    n_cov = sum(int(c.sum()) for c in covered)
    n_near = sum(int(m.sum()) for m in near)
    worst, n_diff = 0, 0
    for x, y, m in zip(a, b, near):
        d = np.abs(x.astype(np.int64) - y.astype(np.int64)).max(axis=2)
        d[m] = 0
        worst, n_diff = max(worst, int(d.max())), n_diff + int((d > 0).sum())
    assert n_cov > 0 and n_near <= 0.005 * n_cov, (n_near, n_cov)
    assert worst <= 1 and n_diff <= 0.005 * n_cov, (worst, n_diff, n_cov)
    return n_diff, worst, n_near, n_cov


# ---- the kernel case at So = S = 16: every way an aligned frame can meet a photo ---------------------------------------------------
# Photos 0..2 are 23 x 37, 40 x 40 and 9 x 64 (odd widths: photo rows start at any byte); photo 3 has no row.  The rows are given as
# BACKWARD maps (aligned pixel -> photo pixel), s = B (i, j) + t.  Rows 1, 3 and 5 overlap each other on photo 1 and are given out of
# spatial order, with rows of other photos between them.
KERNEL_PHOTOS = [(23, 37), (40, 40), (9, 64), (7, 5)]
OVERLAPPING = (1, 3, 5)
TRANSLATION_ROW, SINGULAR_ROW, OUTSIDE_ROW, BAD_IMAGE_ROWS = 0, 10, 9, (11, 12)


def _similarity(deg, scale, cy, cx, reflect=False):
    """(B, t): rotation by deg and scale about the frame centre (7.5, 7.5), which lands on (cy, cx); reflect: det < 0."""
    th = np.deg2rad(deg)
    B = scale * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    if reflect:
        B = B @ np.diag([1.0, -1.0])
    return B, np.array([cy, cx]) - B @ np.array([7.5, 7.5])


def _affine(B, cy, cx):
    B = np.array(B, dtype=np.float64)
    return B, np.array([cy, cx]) - B @ np.array([7.5, 7.5])


KERNEL_MAPS = [
    (0, (np.eye(2), np.array([3.0, 5.0]))),                 # 0   an exact integer translation: the identity case
    (1, _similarity(30.0, 1.0, 13.0, 13.0)),                # 1   rotation 30 degrees; overlap A
    (2, _similarity(10.0, 0.4, 4.5, 12.0)),                 # 2   minification: the face 2.5 x smaller in the photo
    (1, _similarity(-75.0, 1.1, 19.0, 20.0)),               # 3   rotation -75 degrees; overlap B
    (0, _affine([[0.9, 0.35], [-0.2, 1.1]], 12.0, 26.0)),   # 4   a sheared affine map (over a corner of row 0)
    (1, _similarity(180.0, 1.0, 24.0, 16.0)),               # 5   rotation 180 degrees; overlap C
    (0, _similarity(20.0, 0.8, 14.0, 10.0, reflect=True)),  # 6   a reflection: det < 0 (over rows 0 and 4)
    (2, _similarity(15.0, 1.8, 4.5, 45.0)),                 # 7   magnification 1.8 x, over the top and the bottom edge
    (1, _similarity(20.0, 1.0, 38.5, 1.0)),                 # 8   over the bottom left corner of the photo
    (1, _similarity(40.0, 1.0, 80.0, 90.0)),                # 9   wholly outside
    (0, (np.array([[1.0, 2.0], [0.5, 1.0]]), np.array([2.0, 3.0]))),      # 10  singular: det == 0 exactly
    (7, _similarity(5.0, 1.0, 10.0, 10.0)),                 # 11  an image index past the last photo
    (-1, _similarity(5.0, 1.0, 10.0, 10.0)),                # 12  a negative image index
]
# Seed for which unalign_f32 and unalign_f64 meet the cap for every feather of the tests: checked on the CPU by
# test_unalign_cpu.test_f32_restatement_against_f64
KERNEL_SEED = 7


def coefficients_of(B, t, S, So, scale=(1.0, 1.0)):
    """(coef f32 [3, 2], geom f32 [4]) whose backward map is (B, t) up to the f32 rounding of the values: geom = (round(t), scale),
    coef solved from the header's formulas."""
    g = np.array([np.rint(t[0]), np.rint(t[1]), scale[0], scale[1]], dtype=np.float64)
    coef = np.zeros((3, 2))
    for a in range(2):
        k = g[2 + a] * S
        coef[1, a], coef[2, a] = B[a][0] * So / k, B[a][1] * So / k
        coef[0, a] = (t[a] - g[a]) / (k / 2.0) - 1.0 + coef[1, a] + coef[2, a]
    return coef.astype(np.float32), g.astype(np.float32)


def kernel_case(seed=KERNEL_SEED, ld=3):
    """(photos, boxes int32 [n, 5] (only the image index means anything), coef f32 [n, 3, 2], geom f32 [n, 4], faces f32
    [n, 16, 16, ld]): random u8 photos (photo 3 grey), faces uniform in [-60, 315] (so some values clip at either end); the channels
    beyond the third hold NaN, which a kernel that read them would carry into the photo."""
    S = S_KERNEL
    rng = np.random.RandomState(seed)
    photos = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in KERNEL_PHOTOS]
    photos[3] = np.repeat(photos[3][:, :, :1], 3, axis=2)
    n = len(KERNEL_MAPS)
    boxes = np.zeros((n, 5), dtype=np.int32)
    boxes[:, 0] = [i for i, _m in KERNEL_MAPS]
    boxes[:, 3:] = 1
    pairs = [coefficients_of(B, t, S, S, (1.0, 1.0) if b in (TRANSLATION_ROW, SINGULAR_ROW) else (1.25, 0.75))
             for b, (_i, (B, t)) in enumerate(KERNEL_MAPS)]
    coef, geom = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    faces = np.full((n, S, S, ld), np.nan, dtype=np.float32)
    faces[..., :3] = rng.uniform(-60.0, 315.0, size=(n, S, S, 3)).astype(np.float32)
    return photos, boxes, coef, geom, faces


def hw_of(photos):
    return np.array([p.shape[:2] for p in photos], dtype=np.int32)


def float_crop(photo, y0, x0, S):
    """The S x S window at (y0, x0) of a photo as f32 [S, S, 3] (the aligned face of the identity case)."""
    assert y0 >= 0 and x0 >= 0 and y0 + S <= photo.shape[0] and x0 + S <= photo.shape[1]
    return photo[y0:y0 + S, x0:x0 + S].astype(np.float32)
