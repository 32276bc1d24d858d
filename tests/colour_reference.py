"""The rule of imm_colour_stats_u8 / imm_colour_gain / imm_morph_colour_u8 (include/imm_colour.h) restated in numpy.

region          the bool mask of a row's region in its photo: the integer ellipse test of the header, in int64
stats           uint64 [n, 7] from the masks: what the kernel must equal as integers
ellipse_f64     the same ellipse written from its formula in float64 (the brute-force witness of the integer test)
gain            (gain f32 [n, 3, 2], flags int32 [n]) in float64 in the kernel's operation order (numpy rounds every operation
                separately; division and sqrt are correctly rounded on both sides): what the kernel must equal bit for bit
morph_f64 / morph_f32   morph_reference's two restatements with the gain step between the donor's sample and the mix
and the shared inputs of the kernel tests (tests/test_colour_cpu.py, tests/test_colour_gpu.py)."""
import numpy as np

import morph_reference as R
import warp_reference as WR
from morph_reference import _active, _sample_f32, _sample_f64
from warp_reference import U, _box_pixels

MAX_AREA = 1 << 30


def region(row, n_images, hw):
    """row (image, y0, x0, y1, x1), hw [n_images, 2] -> (bool [h, w] of the row's region in its photo, or None for the empty region of a
    row without a photo, with an empty box or with H W > 2^30)."""
    img, y0, x0, y1, x1 = (int(v) for v in row)
    H, W = y1 - y0, x1 - x0
    if img < 0 or img >= n_images or H <= 0 or W <= 0 or H * W > MAX_AREA:
        return None
    h, w = int(hw[img][0]), int(hw[img][1])
    r, c = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    inside = (r >= y0) & (r < y1) & (c >= x0) & (c < x1)
    a, b = 2 * (r - y0) + 1 - H, 2 * (c - x0) + 1 - W
    # outside the box a and b are not bounded by H and W: masked first, so that no product leaves 64 bits
    a, b = np.where(inside, a, 0), np.where(inside, b, 0)
    ea, eb = a * W, b * H
    return inside & (ea * ea + eb * eb <= (H * W) ** 2)


def stats(photos, rows):
    """photos: list of u8 [h, w, 3]; rows int [n, 5] -> uint64 [n, 7]: sum v (3), sum v * v (3), count."""
    hw = [p.shape[:2] for p in photos]
    out = np.zeros((len(rows), 7), dtype=np.uint64)
    for b, row in enumerate(np.asarray(rows).tolist()):
        m = region(row, len(photos), hw)
        if m is None or not m.any():
            continue
        v = photos[row[0]][m].astype(np.uint64)                              # [count, 3]
        out[b, 0:3], out[b, 3:6], out[b, 6] = v.sum(axis=0), (v * v).sum(axis=0), len(v)
    return out


def ellipse_f64(H, W):
    """(inside bool [H, W], margin f64 [H, W]) of a box of H x W pixels from the formula in float64: the pixel centre (i + 0.5, j + 0.5)
    against ((y - H / 2) / (H / 2))^2 + ((x - W / 2) / (W / 2))^2 <= 1; margin = that sum - 1."""
    i, j = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    s = ((i + 0.5 - H / 2.0) / (H / 2.0)) ** 2 + ((j + 0.5 - W / 2.0) / (W / 2.0)) ** 2
    return s <= 1.0, s - 1.0


def moments(sums):
    """uint64 [n, 7] -> (count f64 [n], mean f64 [n, 3], standard deviation f64 [n, 3]) in the gain rule's order; a row without pixels
    gives count 0 and NaN."""
    s = np.asarray(sums).astype(np.uint64)
    N = s[:, 6].astype(np.float64)[:, None]
    with np.errstate(all='ignore'):
        m, q = s[:, 0:3].astype(np.float64) / N, s[:, 3:6].astype(np.float64) / N
        sd = np.sqrt(np.maximum(q - m * m, 0.0))
    return N[:, 0], m, sd


def gain(sums_a, sums_b, amount, max_gain):
    """-> (gain f32 [n, 3, 2], flags int32 [n]) in the header's operation order."""
    f64 = np.float64
    Na, ma, sda = moments(sums_a)
    Nb, mb, sdb = moments(sums_b)
    t = np.asarray(amount, dtype=np.float32).astype(f64)
    flagged = (Na == 0) | (Nb == 0) | ~np.isfinite(t)
    with np.errstate(all='ignore'):
        g = np.where(sdb > 0.0, sda / np.where(sdb > 0.0, sdb, 1.0), 1.0)
        g = np.minimum(np.maximum(g, f64(1.0) / f64(max_gain)), f64(max_gain))
        gm = g * mb
        o = ma - gm
        tg, to = t[:, None] * (g - 1.0), t[:, None] * o
        G, O = (1.0 + tg).astype(np.float32), to.astype(np.float32)
    out = np.stack([G, O], axis=2)
    out[flagged] = (1.0, 0.0)
    return out, flagged.astype(np.int32)


def morph_f64(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, inv_ramp, gain):
    """morph_reference.morph_f64 with gB' = gB G + O (the f32 gain widened) in front of the mix."""
    out = [np.array(p, dtype=np.uint8, copy=True) for p in photos]
    covered = [np.zeros(p.shape[:2], dtype=bool) for p in photos]
    ctrl, coef_a, coef_b, inv_ramp, texture = (np.asarray(a, dtype=np.float64) for a in (ctrl, coef_a, coef_b, inv_ramp, texture))
    gain = np.asarray(gain, dtype=np.float32).astype(np.float64)
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
        gB = gB * gain[b, :, 0][None, :] + gain[b, :, 1][None, :]
        mix = (1.0 - texture[b]) * gA + texture[b] * gB
        wy = np.minimum(1.0, (np.minimum(r - y0, y1 - 1 - r) + 0.5) * inv_ramp[b, 0])
        wx = np.minimum(1.0, (np.minimum(c - x0, x1 - 1 - c) + 0.5) * inv_ramp[b, 1])
        a = (wy * wx)[:, None]
        p = ph[r, c].astype(np.float64)
        ph[r, c] = np.clip(np.rint((1 - a) * p + a * mix), 0, 255).astype(np.uint8)
        covered[img][r, c] = True
    return out, covered


def morph_f32(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, inv_ramp, gain):
    """morph_reference.morph_f32 with the kernel's added step: sc = gB * G, gB' = sc + O, every operation rounded to f32."""
    f32 = np.float32
    out = [np.array(p, dtype=np.uint8, copy=True) for p in photos]
    covered = [np.zeros(p.shape[:2], dtype=bool) for p in photos]
    ctrl, ca, cb, inv_ramp, texture, gain = (np.asarray(a, dtype=f32) for a in (ctrl, coef_a, coef_b, inv_ramp, texture, gain))
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
        ok = np.isfinite(ay) & np.isfinite(ax) & np.isfinite(by) & np.isfinite(bx)
        if not ok.any():
            continue
        r, c = r[ok], c[ok]
        gA, gB = _sample_f32(src, ay[ok], ax[ok]), _sample_f32(don, by[ok], bx[ok])
        with np.errstate(all='ignore'):
            sc = gB * gain[b, :, 0][None, :]
            gB = sc + gain[b, :, 1][None, :]
            e = gB - gA
            te = texture[b] * e
            mix = gA + te
            wy = np.minimum(f32(1), (np.minimum(r - y0, y1 - 1 - r).astype(f32) + f32(0.5)) * inv_ramp[b, 0])
            wx = np.minimum(f32(1), (np.minimum(c - x0, x1 - 1 - c).astype(f32) + f32(0.5)) * inv_ramp[b, 1])
            a = (wy * wx)[:, None]
            p = ph[r, c].astype(f32)
            d = mix - p
            mm = a * d
            # the kernel's fminf(fmaxf(x, 0), 255) returns the other operand for a NaN: 0
            v = np.fmin(np.fmax(np.rint(p + mm), f32(0)), f32(255))
        assert v.dtype == f32 and gB.dtype == f32
        ph[r, c] = v.astype(np.uint8)
        covered[img][r, c] = True
    return out, covered


# ---- the kernel cases ---------------------------------------------------------------------------------------------------------------
# Stats: photos of odd widths (a photo row starts at any byte) and boxes of every kind the issue names.
STATS_PHOTOS = [(37, 53), (64, 70), (9, 11)]
STATS_ROWS = [
    (0, 5, 9, 6, 10),             # 0   1 x 1
    (0, 20, 3, 21, 10),           # 1   1 x 7
    (2, 3, 4, 5, 6),              # 2   2 x 2
    (0, 10, 20, 27, 43),          # 3   17 x 23
    (1, 0, 3, 64, 67),            # 4   64 x 64: more than one block
    (0, -6, 40, 14, 60),          # 5   over the top and the right edge of the photo
    (2, 4, -5, 20, 8),            # 6   over the bottom and the left edge
    (0, 100, 100, 120, 130),      # 7   wholly outside
    (0, -2000000000, 0, -1999999990, 10),     # 8   wholly outside, far
    (1, 10, 10, 10, 30),          # 9   empty: H == 0
    (1, 30, 10, 20, 5),           # 10  empty: negative sides
    (-1, 0, 0, 10, 10),           # 11  image index -1
    (3, 0, 0, 10, 10),            # 12  image index n_images
    (1, -40000, -40000, 40000, 40000),        # 13  H W > 2^30: the empty region by rule, although it covers the photo
    (1, -10, -10, 74, 80),        # 14  the whole photo inside the ellipse's bounding box
    (0, -2147483648, 5, 2147483647, 6),       # 15  one pixel wide and 2^32 - 1 tall: H W > 2^30, sides beyond 32 bits
]
STATS_SEED = 5


def stats_photos(seed=STATS_SEED):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in STATS_PHOTOS]


def stats_rows(n, seed=STATS_SEED):
    """n box rows: the first of STATS_ROWS, then random boxes (some over an edge) on the three photos."""
    rng = np.random.RandomState(seed + n)
    rows = [tuple(r) for r in STATS_ROWS[:n]]
    while len(rows) < n:
        img = int(rng.randint(0, len(STATS_PHOTOS)))
        h, w = STATS_PHOTOS[img]
        y0, x0 = int(rng.randint(-5, h)), int(rng.randint(-5, w))
        rows.append((img, y0, x0, y0 + int(rng.randint(1, 40)), x0 + int(rng.randint(1, 40))))
    return np.array(rows, dtype=np.int32)


def flat_photo(h, w, colour):
    p = np.empty((h, w, 3), dtype=np.uint8)
    p[:] = colour
    return p


# Morph with colour: morph_reference's kernel case (photos, rows, donors, donor rows, landmarks, shape, texture) with amounts of its own;
# the gains come from the rule at MAX_GAIN on the two sides' statistics.
MAX_GAIN = 2.0
AMOUNT_ZERO_ROW, AMOUNT_ONE_ROW = 2, 4


def morph_gains(case, seed=R.KERNEL_SEED):
    """(gain f32 [n, 3, 2], flags, amount f32 [n]) of morph_reference.kernel_case's rows."""
    photos, rows, donors, drows = case[:4]
    rng = np.random.RandomState(seed + 900)
    amount = rng.uniform(0.1, 1.0, len(rows)).astype(np.float32)
    amount[AMOUNT_ZERO_ROW], amount[AMOUNT_ONE_ROW] = 0.0, 1.0
    g, flags = gain(stats(photos, rows), stats(donors, drows), amount, MAX_GAIN)
    return g, flags, amount


def inv_ramp(rows, feather):
    return WR.inv_ramp(rows, feather)
