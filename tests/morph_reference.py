"""The rule of imm_morph_poses / imm_morph_u8 (include/imm_morph.h) restated in numpy: morph_f64, the morph in float64 written from the
formulas (tap weights (1 - t), t; mix (1 - texture) gA + texture gB; blend (1 - a) p + a mix); morph_f32, the morph in float32 in the
kernel's operation order (numpy rounds every f32 operation separately, as the kernel's unfused arithmetic does; only its log is another
implementation than the device's).  Both sample the ORIGINAL photos and the donor photos, apply the rows in row order, round to u8
after every row and return the mask of the pixels some row wrote.  The fit is warp_reference.fit_f64 over the 2 n rows (poses, poses)
against (mu_a, mu_b).  Also the shared inputs of the kernel tests (tests/test_morph_cpu.py, tests/test_morph_gpu.py): warp_reference's
photos and box rows with donor photos, donor box rows, two sets of landmarks, shapes and textures of their own."""
import numpy as np

import warp_reference as WR
from alignment_reference import smooth_photo
from warp_reference import U, _box_pixels


def blend_f64(mu_a, mu_b, shape):
    """(1 - s) mu_a + s mu_b in float64 from the f32 inputs widened."""
    a, b = np.asarray(mu_a, np.float32).astype(np.float64), np.asarray(mu_b, np.float32).astype(np.float64)
    s = np.asarray(shape, np.float32).astype(np.float64)[:, None, None]
    return (1.0 - s) * a + s * b


def blend_f32(mu_a, mu_b, shape):
    """The kernel's order in f32: wa = 1 - s, then wa * mu_a + s * mu_b, every operation rounded."""
    f32 = np.float32
    a, b, s = np.asarray(mu_a, f32), np.asarray(mu_b, f32), np.asarray(shape, f32)[:, None, None]
    with np.errstate(all='ignore'):
        wa = f32(1) - s
        ta = wa * a
        tb = s * b
        out = ta + tb
    assert out.dtype == f32
    return out


def fit2_f64(mu_a, mu_b, poses, m, lam):
    """The two displacement splines of every row on the shared control points (poses, anchors): (coef_a, coef_b f64 [n, M + 3, 2],
    ctrl f32 [n, M, 2], flags int [n] (the OR of the two), cond [n])."""
    n = len(poses)
    coef, ctrl, flags, cond = WR.fit_f64(np.concatenate([poses, poses]), np.concatenate([mu_a, mu_b]), m, 1.0, lam)
    return coef[:n], coef[n:], ctrl[:n], flags[:n] | flags[n:], np.maximum(cond[:n], cond[n:])


def _active(drow, n_donors):
    img, y0, x0, y1, x1 = drow
    return 0 <= img < n_donors and y1 - y0 > 0 and x1 - x0 > 0


def _sample_f64(photo, sy, sx):
    h, w = photo.shape[:2]
    fy, fx = np.floor(sy), np.floor(sx)
    ty, tx = (sy - fy)[:, None], (sx - fx)[:, None]
    yl, yh = np.clip(fy, 0, h - 1).astype(np.int64), np.clip(fy + 1, 0, h - 1).astype(np.int64)
    xl, xh = np.clip(fx, 0, w - 1).astype(np.int64), np.clip(fx + 1, 0, w - 1).astype(np.int64)
    s = photo.astype(np.float64)
    return (1 - ty) * ((1 - tx) * s[yl, xl] + tx * s[yl, xh]) + ty * ((1 - tx) * s[yh, xl] + tx * s[yh, xh])


def morph_f64(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, inv_ramp):
    """photos, donors: lists of u8 [h, w, 3]; rows, drows int [n, 5]; ctrl [n, M, 2], coef_a, coef_b [n, M + 3, 2] (the values given,
    widened); texture [n]; inv_ramp [n, 2] -> (new photos, per photo a bool [h, w] of the pixels some row WROTE: inside a box of an
    active row, where all four source coordinates are finite).  Float64, from the formulas: q = 2 (r - y0) / H - 1, DA(q), DB(q),
    sA = (r, c) + (H / 2, W / 2) DA, sB = (y0_B, x0_B) + (q + DB + 1) (H_B / 2, W_B / 2)."""
    out = [np.array(p, dtype=np.uint8, copy=True) for p in photos]
    covered = [np.zeros(p.shape[:2], dtype=bool) for p in photos]
    ctrl, coef_a, coef_b, inv_ramp, texture = (np.asarray(a, dtype=np.float64) for a in (ctrl, coef_a, coef_b, inv_ramp, texture))
    M = ctrl.shape[1]
    for b, (row, drow) in enumerate(zip(np.asarray(rows).tolist(), np.asarray(drows).tolist())):
        img, y0, x0, y1, x1 = row
        if img < 0 or img >= len(out) or not _active(drow, len(donors)):
            continue
        src, ph, don = photos[img], out[img], donors[drow[0]]
        px = _box_pixels(row, *ph.shape[:2])
        if px is None:
            continue
        r, c = px
        H, W = float(y1 - y0), float(x1 - x0)
        HB, WB = float(drow[3] - drow[1]), float(drow[4] - drow[2])
        q = np.stack([2.0 * (r - y0) / H - 1.0, 2.0 * (c - x0) / W - 1.0], axis=1)
        d = q[:, None, :] - ctrl[b][None, :, :]
        u = U((d * d).sum(axis=-1))
        with np.errstate(all='ignore'):
            DA = u @ coef_a[b, :M] + coef_a[b, M] + q[:, :1] * coef_a[b, M + 1] + q[:, 1:] * coef_a[b, M + 2]
            DB = u @ coef_b[b, :M] + coef_b[b, M] + q[:, :1] * coef_b[b, M + 1] + q[:, 1:] * coef_b[b, M + 2]
            ay, ax = r + H / 2.0 * DA[:, 0], c + W / 2.0 * DA[:, 1]
            by, bx = drow[1] + (q[:, 0] + DB[:, 0] + 1.0) * HB / 2.0, drow[2] + (q[:, 1] + DB[:, 1] + 1.0) * WB / 2.0
        ok = np.isfinite(ay) & np.isfinite(ax) & np.isfinite(by) & np.isfinite(bx)
        if not ok.any():
            continue
        r, c = r[ok], c[ok]
        gA, gB = _sample_f64(src, ay[ok], ax[ok]), _sample_f64(don, by[ok], bx[ok])
        mix = (1.0 - texture[b]) * gA + texture[b] * gB
        wy = np.minimum(1.0, (np.minimum(r - y0, y1 - 1 - r) + 0.5) * inv_ramp[b, 0])
        wx = np.minimum(1.0, (np.minimum(c - x0, x1 - 1 - c) + 0.5) * inv_ramp[b, 1])
        a = (wy * wx)[:, None]
        p = ph[r, c].astype(np.float64)
        ph[r, c] = np.clip(np.rint((1 - a) * p + a * mix), 0, 255).astype(np.uint8)
        covered[img][r, c] = True
    return out, covered


def _sample_f32(photo, sy, sx):
    f32 = np.float32
    h, w = photo.shape[:2]
    fy, fx = np.floor(sy), np.floor(sx)
    ty, tx = (sy - fy)[:, None], (sx - fx)[:, None]
    iy = np.minimum(np.maximum(fy, f32(-1)), f32(h)).astype(np.int64)
    ix = np.minimum(np.maximum(fx, f32(-1)), f32(w)).astype(np.int64)
    yl, yh = np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
    xl, xh = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1)
    s = photo.astype(f32)
    tl, tr, bl, br = s[yl, xl], s[yl, xh], s[yh, xl], s[yh, xh]
    top = tl + (tr - tl) * tx
    bot = bl + (br - bl) * tx
    g = top + (bot - top) * ty
    assert g.dtype == f32
    return g


def morph_f32(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, inv_ramp):
    """The same in float32 in the kernel's operation order -> (new photos, covered)."""
    f32 = np.float32
    out = [np.array(p, dtype=np.uint8, copy=True) for p in photos]
    covered = [np.zeros(p.shape[:2], dtype=bool) for p in photos]
    ctrl, ca, cb, inv_ramp, texture = (np.asarray(a, dtype=f32) for a in (ctrl, coef_a, coef_b, inv_ramp, texture))
    M = ctrl.shape[1]
    for b, (row, drow) in enumerate(zip(np.asarray(rows).tolist(), np.asarray(drows).tolist())):
        img, y0, x0, y1, x1 = row
        if img < 0 or img >= len(out) or not _active(drow, len(donors)):
            continue
        src, ph, don = photos[img], out[img], donors[drow[0]]
        px = _box_pixels(row, *ph.shape[:2])
        if px is None:
            continue
        r, c = px
        ih, iw = y1 - y0, x1 - x0
        ry, rx = f32(2.0 / np.float64(ih)), f32(2.0 / np.float64(iw))
        hy, hx = f32(0.5) * f32(ih), f32(0.5) * f32(iw)
        oy, ox = f32(drow[1]), f32(drow[2])
        dhy, dhx = f32(0.5) * f32(drow[3] - drow[1]), f32(0.5) * f32(drow[4] - drow[2])
        qy, qx = (r - y0).astype(f32) * ry - f32(1), (c - x0).astype(f32) * rx - f32(1)
        Ay, Ax, By, Bx = (np.zeros(len(r), dtype=f32) for _ in range(4))
        with np.errstate(all='ignore'):
            for j in range(M):
                dy, dx = qy - ctrl[b, j, 0], qx - ctrl[b, j, 1]
                d2 = dy * dy + dx * dx
                u = np.where(d2 > 0, d2 * np.log(np.where(d2 > 0, d2, f32(1))), f32(0)).astype(f32)
                Ay = Ay + ca[b, j, 0] * u
                Ax = Ax + ca[b, j, 1] * u
                By = By + cb[b, j, 0] * u
                Bx = Bx + cb[b, j, 1] * u
            Ay = ((Ay + ca[b, M, 0]) + ca[b, M + 1, 0] * qy) + ca[b, M + 2, 0] * qx
            Ax = ((Ax + ca[b, M, 1]) + ca[b, M + 1, 1] * qy) + ca[b, M + 2, 1] * qx
            By = ((By + cb[b, M, 0]) + cb[b, M + 1, 0] * qy) + cb[b, M + 2, 0] * qx
            Bx = ((Bx + cb[b, M, 1]) + cb[b, M + 1, 1] * qy) + cb[b, M + 2, 1] * qx
            ay, ax = r.astype(f32) + hy * Ay, c.astype(f32) + hx * Ax
            by, bx = oy + ((qy + By) + f32(1)) * dhy, ox + ((qx + Bx) + f32(1)) * dhx
        assert ay.dtype == f32 and ax.dtype == f32 and by.dtype == f32 and bx.dtype == f32
        ok = np.isfinite(ay) & np.isfinite(ax) & np.isfinite(by) & np.isfinite(bx)
        if not ok.any():
            continue
        r, c = r[ok], c[ok]
        gA, gB = _sample_f32(src, ay[ok], ax[ok]), _sample_f32(don, by[ok], bx[ok])
        e = gB - gA
        te = texture[b] * e
        mix = gA + te
        wy = np.minimum(f32(1), (np.minimum(r - y0, y1 - 1 - r).astype(f32) + f32(0.5)) * inv_ramp[b, 0])
        wx = np.minimum(f32(1), (np.minimum(c - x0, x1 - 1 - c).astype(f32) + f32(0.5)) * inv_ramp[b, 1])
        a = (wy * wx)[:, None]
        p = ph[r, c].astype(f32)
        d = mix - p
        mm = a * d
        v = np.minimum(np.maximum(np.rint(p + mm), f32(0)), f32(255))
        assert v.dtype == f32
        ph[r, c] = v.astype(np.uint8)
        covered[img][r, c] = True
    return out, covered


# ---- the kernel case --------------------------------------------------------------------------------------------------------------
# The own side is warp_reference's: KERNEL_PHOTOS and KERNEL_ROWS (row 13, whose OWN image index is out of range, stays the check of
# the own side).  The donor side: three photos of other sizes and fifteen box rows with sides from 5 to 40 px and aspect ratios unlike
# the own boxes'.  Rows 8 and 11 reach outside their donor photo (the taps are clamped).  Row 6 names a donor photo that does not exist:
# its own box is valid, lies wholly under row 4 and is the middle one of the three overlapping rows, so the walks have to pass over it.
DONOR_PHOTOS = [(31, 29), (40, 40), (12, 50)]
DONOR_ROWS = [
    (0, 2, 3, 27, 23),        # 0   25 x 20 for a 16 x 16 box; mu_b == mu_a
    (2, 1, 5, 11, 45),        # 1   10 x 40 for 1 x 9
    (1, 5, 8, 25, 38),        # 2   20 x 30 for 18 x 24
    (0, 10, 5, 30, 15),       # 3   20 x 10 for 14 x 12
    (1, 0, 0, 40, 40),        # 4   the whole 40 x 40 photo for 40 x 31
    (2, 3, 20, 9, 30),        # 5   6 x 10 (the NaN row)
    (5, 2, 2, 22, 17),        # 6   a donor image index past the last donor photo
    (0, 4, 4, 9, 29),         # 7   5 x 25 for 9 x 1
    (1, -6, 20, 18, 45),      # 8   over the top and the right edge of the donor photo
    (0, 0, 0, 20, 20),        # 9   (the own box is wholly outside)
    (2, 0, 10, 12, 45),       # 10  12 x 35 for 20 x 18
    (0, 20, -4, 36, 12),      # 11  over the bottom and the left edge of the donor photo
    (1, 10, 10, 18, 33),      # 12  8 x 23 for 9 x 12
    (0, 1, 1, 11, 21),        # 13  (the own image index is out of range)
    (1, 1, 1, 21, 11),        # 14  (the own image index is negative)
]
BAD_DONOR_ROW, DONOR_OUTSIDE_ROWS = 6, (8, 11)
IDENTITY_ROW, NAN_ROW, OUTSIDE_ROW, BAD_IMAGE_ROWS = WR.IDENTITY_ROW, WR.NAN_ROW, WR.OUTSIDE_ROW, WR.BAD_IMAGE_ROWS
SILENT_ROWS = (NAN_ROW, OUTSIDE_ROW, BAD_DONOR_ROW) + tuple(BAD_IMAGE_ROWS)            # the rows that write nothing
SHAPE_ZERO_ROW, SHAPE_ONE_ROW, TEXTURE_ZERO_ROW, TEXTURE_ONE_ROW = 3, 8, 1, 11
KERNEL_SHAPES, LAMS, FEATHERS = WR.KERNEL_SHAPES, WR.LAMS, WR.FEATHERS
# Seed for which morph_f32 stays at or below half the cap's share against morph_f64 for every shape, lam and feather of the tests and
# the condition numbers stay <= 1e4: checked on the CPU by test_morph_cpu.test_f32_restatement_against_f64
KERNEL_SEED = 7


def landmarks(K, n, rng):
    """(mu_a, mu_b) f32 [n, K, 2]: per row K cells of the grid of warp_reference.landmarks over [-0.8, 0.8]^2 (cells of side
    1.6 / ceil(sqrt(K))), and both landmark sets = the cell centres + N(0, cell / 8) each: every blend of the two stays near its
    centre, so the blended control points stay apart and the systems well conditioned."""
    g = int(np.ceil(np.sqrt(K)))
    cell = 1.6 / g
    centre = np.zeros((n, K, 2))
    for b in range(n):
        pick = rng.permutation(g * g)[:K]
        centre[b] = np.stack([pick // g, pick % g], axis=1) * cell - 0.8 + cell / 2
    mu_a = centre + rng.normal(0.0, cell / 8, size=centre.shape)
    mu_b = centre + rng.normal(0.0, cell / 8, size=centre.shape)
    return mu_a.astype(np.float32), mu_b.astype(np.float32)


def donor_photos(K, seed):
    """Uniform-noise donor photos for K <= 10, smooth ones above (as warp_reference.kernel_photos)."""
    rng = np.random.RandomState(seed + 2000)
    if K <= 10:
        return [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in DONOR_PHOTOS]
    return [smooth_photo(h, w, seed + 50 + i) for i, (h, w) in enumerate(DONOR_PHOTOS)]


def kernel_case(K, m, seed=KERNEL_SEED):
    """(photos, rows int32 [n, 5], donors, drows int32 [n, 5], mu_a, mu_b f32 [n, K, 2], shape f32 [n], texture f32 [n])."""
    rng = np.random.RandomState(seed + 37 * K)
    rows, drows = np.array(WR.KERNEL_ROWS, dtype=np.int32), np.array(DONOR_ROWS, dtype=np.int32)
    n = len(rows)
    mu_a, mu_b = landmarks(K, n, rng)
    mu_b[IDENTITY_ROW] = mu_a[IDENTITY_ROW]
    mu_a[NAN_ROW, K // 2, 1] = np.nan
    shape, texture = rng.uniform(0.05, 0.95, n).astype(np.float32), rng.uniform(0.05, 0.95, n).astype(np.float32)
    shape[SHAPE_ZERO_ROW], shape[SHAPE_ONE_ROW] = 0.0, 1.0
    texture[TEXTURE_ZERO_ROW], texture[TEXTURE_ONE_ROW] = 0.0, 1.0
    return WR.kernel_photos(K, seed), rows, donor_photos(K, seed), drows, mu_a, mu_b, shape, texture


def fitted_case(K, m, lam, seed=KERNEL_SEED):
    """kernel_case with its poses and its f64 fit: (case, poses f32, coef_a, coef_b f64, ctrl f32, flags, cond)."""
    case = kernel_case(K, m, seed)
    poses = blend_f32(case[4], case[5], case[6])
    return (case, poses) + fit2_f64(case[4], case[5], poses, m, lam)
