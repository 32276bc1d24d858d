"""The rule of imm_seam_fit / imm_morph_seam_u8 (include/imm_seam.h) restated in numpy.

ring_f64        (ring f32 [n, B, 2], flags int32 [n]) in float64 in the kernel's operation order (numpy rounds every operation separately;
                division is correctly rounded on both sides): what the kernel must equal bit for bit
diff_f32        the differences at the ring's samples in the kernel's f32 order (only its log is another implementation than the
                device's); diff_f64 the same in float64 from the formulas
field           the membrane at box-relative pixel places, in the rule's order, in float32 (the kernel's bits: sqrt and division are
                correctly rounded on both sides) or in float64 from the f32 ring and diffs widened
morph_seam_f32 / morph_seam_f64   hull_reference's two restatements of the morph with the mask, with seamless * field added to the mix
and the shared inputs of the kernel tests (tests/test_seam_cpu.py, tests/test_seam_gpu.py)."""
import numpy as np

import hull_reference as HR
import morph_reference as R
import warp_reference as WR
from morph_reference import _active, _sample_f32, _sample_f64
from warp_reference import U, _box_pixels

F32, F64 = np.float32, np.float64


def dirs(B):
    """The host's dirs f64 [B, 2]: (cos, sin) of 2 pi s / B."""
    a = 2.0 * np.pi * np.arange(B, dtype=F64) / F64(B)
    return np.stack([np.cos(a), np.sin(a)], axis=1)


def ring_f64(poses, rows, edges, hull_flags, dirs_):
    """poses f32 [n, K, 2], rows int [n, 5], edges f32 [n, K, 3], hull_flags int [n], dirs f64 [B, 2] -> (ring f32 [n, B, 2], flags int32
    [n]) in the header's operation order."""
    p, e = np.asarray(poses, F32).astype(F64), np.asarray(edges, F32).astype(F64)
    n, K = p.shape[:2]
    rows = np.asarray(rows).reshape(-1, 5)
    uy, ux = np.asarray(dirs_, F64)[:, 0], np.asarray(dirs_, F64)[:, 1]
    B = len(uy)
    ring, flags = np.zeros((n, B, 2), F32), np.zeros(n, np.int32)
    for b in range(n):
        H, W = F64(int(rows[b, 3]) - int(rows[b, 1])), F64(int(rows[b, 4]) - int(rows[b, 2]))
        with np.errstate(all='ignore'):
            vy, vx = (p[b, :, 0] + 1.0) * (0.5 * H), (p[b, :, 1] + 1.0) * (0.5 * W)
            sy, sx = vy[0], vx[0]
            for i in range(1, K):                                              # in index order
                sy, sx = sy + vy[i], sx + vx[i]
            cy, cx = sy / F64(K), sx / F64(K)
            lines = list(e[b]) + [(1.0, 0.0, 0.0), (-1.0, 0.0, H - 1.0), (0.0, 1.0, 0.0), (0.0, -1.0, W - 1.0)]
            bad = bool(hull_flags[b]) or not (np.isfinite(cy) and np.isfinite(cx))
            t = np.full(B, np.inf)
            for ny, nx, d in lines:
                ny, nx, d = F64(ny), F64(nx), F64(d)
                s0 = (ny * cy + nx * cx) + d
                bad = bad or not s0 > 0.0
                g = ny * uy + nx * ux
                t = np.where(g < 0.0, np.fmin(t, s0 / np.where(g < 0.0, -g, 1.0)), t)
            f = int(bad) | 2 * int(not (np.isfinite(t) & (t > 0.0)).all())
            flags[b] = f
            if f:
                ring[b, :, 0], ring[b, :, 1] = F32(cy), F32(cx)
            else:
                ring[b, :, 0], ring[b, :, 1] = (cy + t * uy).astype(F32), (cx + t * ux).astype(F32)
    return ring, flags


def _mix_f32(photos, donors, row, drow, ctrl, ca, cb, tex, gain, fy, fx):
    """The morph's mix at the box-relative places (fy, fx) f32 [N] of one ACTIVE row, in the kernel's f32 order (with integer places:
    morph_reference.morph_f32's) -> (mix f32 [N, 3] (rows that are not ok: undefined), ok bool [N], (oy, ox) the places in the photo)."""
    f32 = F32
    img, y0, x0, y1, x1 = row
    src, don = photos[img], donors[drow[0]]
    M = ctrl.shape[0]
    ih, iw = y1 - y0, x1 - x0
    ry, rx = f32(2.0 / F64(ih)), f32(2.0 / F64(iw))
    hy, hx = f32(0.5) * f32(ih), f32(0.5) * f32(iw)
    oy0, ox0 = f32(drow[1]), f32(drow[2])
    dhy, dhx = f32(0.5) * f32(drow[3] - drow[1]), f32(0.5) * f32(drow[4] - drow[2])
    with np.errstate(all='ignore'):
        qy, qx = fy * ry - f32(1), fx * rx - f32(1)
        Ay, Ax, By, Bx = (np.zeros(len(fy), dtype=f32) for _ in range(4))
        for j in range(M):
            dy, dx = qy - ctrl[j, 0], qx - ctrl[j, 1]
            d2 = dy * dy + dx * dx
            u = np.where(d2 > 0, d2 * np.log(np.where(d2 > 0, d2, f32(1))), f32(0)).astype(f32)
            Ay = Ay + ca[j, 0] * u
            Ax = Ax + ca[j, 1] * u
            By = By + cb[j, 0] * u
            Bx = Bx + cb[j, 1] * u
        Ay = ((Ay + ca[M, 0]) + ca[M + 1, 0] * qy) + ca[M + 2, 0] * qx
        Ax = ((Ax + ca[M, 1]) + ca[M + 1, 1] * qy) + ca[M + 2, 1] * qx
        By = ((By + cb[M, 0]) + cb[M + 1, 0] * qy) + cb[M + 2, 0] * qx
        Bx = ((Bx + cb[M, 1]) + cb[M + 1, 1] * qy) + cb[M + 2, 1] * qx
        oy, ox = f32(y0) + fy, f32(x0) + fx
        ay, ax = oy + hy * Ay, ox + hx * Ax
        by, bx = oy0 + ((qy + By) + f32(1)) * dhy, ox0 + ((qx + Bx) + f32(1)) * dhx
        ok = np.isfinite(ay) & np.isfinite(ax) & np.isfinite(by) & np.isfinite(bx) & np.isfinite(oy) & np.isfinite(ox)
        z = f32(0)
        gA, gB = _sample_f32(src, np.where(ok, ay, z), np.where(ok, ax, z)), _sample_f32(don, np.where(ok, by, z), np.where(ok, bx, z))
        if gain is not None:
            sc = gB * gain[:, 0][None, :]
            gB = sc + gain[:, 1][None, :]
        e = gB - gA
        te = tex * e
        mix = gA + te
    assert mix.dtype == f32 and oy.dtype == f32
    return mix, ok, (oy, ox)


def _mix_f64(photos, donors, row, drow, ctrl, ca, cb, tex, gain, fy, fx):
    """The same in float64, from the formulas (morph_reference.morph_f64's)."""
    img, y0, x0, y1, x1 = row
    src, don = photos[img], donors[drow[0]]
    M = ctrl.shape[0]
    H, W = float(y1 - y0), float(x1 - x0)
    HB, WB = float(drow[3] - drow[1]), float(drow[4] - drow[2])
    with np.errstate(all='ignore'):
        q = np.stack([2.0 * fy / H - 1.0, 2.0 * fx / W - 1.0], axis=1)
        d = q[:, None, :] - ctrl[None, :, :]
        u = U((d * d).sum(axis=-1))
        DA = u @ ca[:M] + ca[M] + q[:, :1] * ca[M + 1] + q[:, 1:] * ca[M + 2]
        DB = u @ cb[:M] + cb[M] + q[:, :1] * cb[M + 1] + q[:, 1:] * cb[M + 2]
        oy, ox = y0 + fy, x0 + fx
        ay, ax = oy + H / 2.0 * DA[:, 0], ox + W / 2.0 * DA[:, 1]
        by, bx = drow[1] + (q[:, 0] + DB[:, 0] + 1.0) * HB / 2.0, drow[2] + (q[:, 1] + DB[:, 1] + 1.0) * WB / 2.0
        ok = np.isfinite(ay) & np.isfinite(ax) & np.isfinite(by) & np.isfinite(bx) & np.isfinite(oy) & np.isfinite(ox)
        gA, gB = _sample_f64(src, np.where(ok, ay, 0.0), np.where(ok, ax, 0.0)), _sample_f64(don, np.where(ok, by, 0.0), np.where(ok, bx, 0.0))
        if gain is not None:
            gB = gB * gain[:, 0][None, :] + gain[:, 1][None, :]
        mix = (1.0 - tex) * gA + tex * gB
    return mix, ok, (oy, ox)


def _pastes(row, drow, photos, donors):
    img = row[0]
    return 0 <= img < len(photos) and _active(drow, len(donors)) and min(photos[img].shape[:2]) > 0 and min(donors[drow[0]].shape[:2]) > 0


def _diff(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, ring, flags, gain, dt):
    mixer, sample = (_mix_f32, _sample_f32) if dt is F32 else (_mix_f64, _sample_f64)
    ctrl, ca, cb, texture, ring = (np.asarray(a, F32).astype(dt) for a in (ctrl, coef_a, coef_b, texture, ring))
    gain = None if gain is None else np.asarray(gain, F32).astype(dt)
    out = np.zeros(ring.shape[:2] + (3,), dt)
    for b, (row, drow) in enumerate(zip(np.asarray(rows).tolist(), np.asarray(drows).tolist())):
        if flags[b] or not _pastes(row, drow, photos, donors):
            continue
        mix, ok, (oy, ox) = mixer(photos, donors, row, drow, ctrl[b], ca[b], cb[b], texture[b], None if gain is None else gain[b],
                                  ring[b, :, 0], ring[b, :, 1])
        with np.errstate(all='ignore'):
            own = sample(photos[row[0]], np.where(ok, oy, dt(0)), np.where(ok, ox, dt(0)))
            out[b] = np.where(ok[:, None], own - mix, dt(0))
    assert out.dtype == dt
    return out


def diff_f32(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, ring, flags, gain=None):
    """diff f32 [n, B, 3] at ring f32 [n, B, 2] in the kernel's f32 order; flags: imm_seam_fit's (a flagged row gets 0)."""
    return _diff(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, ring, flags, gain, F32)


def diff_f64(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, ring, flags, gain=None):
    """The same in float64 from the formulas, from the f32 inputs widened."""
    return _diff(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, ring, flags, gain, F64)


def weights(ring, rr, cc, dt=F64):
    """The mean-value weights w_s [B, N] of the places (rr, cc) [N] in ring [B, 2] and the lengths l_s, in the rule's order, in dt."""
    rg = np.asarray(ring, F32).astype(dt)
    rr, cc = np.asarray(rr).astype(dt), np.asarray(cc).astype(dt)
    B = len(rg)
    with np.errstate(all='ignore'):
        py, px = rg[:, 0, None] - rr[None, :], rg[:, 1, None] - cc[None, :]
        ln = np.sqrt(py * py + px * px)
        nxt = np.roll(np.arange(B), -1)
        cr, dot = py * px[nxt] - px * py[nxt], py * py[nxt] + px * px[nxt]
        th = cr / (ln * ln[nxt] + dot)
        w = (np.roll(th, 1, axis=0) + th) / ln
    assert w.dtype == dt
    return w, ln


def field(ring, diff, rr, cc, dt=F32):
    """r [N, 3] at the box-relative places (rr, cc) [N] from ring f32 [B, 2] and diff f32 [B, 3], in the rule's order, in dt."""
    df = np.asarray(diff, F32).astype(dt)
    w, ln = weights(ring, rr, cc, dt)
    R, Ws = np.zeros((w.shape[1], 3), dt), np.zeros(w.shape[1], dt)
    with np.errstate(all='ignore'):
        for s in range(len(df)):                                               # s = 0 .. B - 1 in order
            R = R + w[s][:, None] * df[s][None, :]
            Ws = Ws + w[s]
        ok = (Ws > 0) & np.isfinite(Ws) & np.isfinite(R).all(axis=1)
        r = np.where(ok[:, None], R / np.where(ok, Ws, dt(1))[:, None], dt(0))
    on = ln == 0
    hit = on.any(axis=0)
    r[hit] = df[np.argmax(on, axis=0)[hit]]
    assert r.dtype == dt
    return r


def _morph_seam(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, inv_ramp, edges, isoft, ring, diff, seamless, gain, dt):
    mixer, weight = (_mix_f32, HR.weight_f32) if dt is F32 else (_mix_f64, HR.weight_f64)
    out = [np.array(p, dtype=np.uint8, copy=True) for p in photos]
    covered = [np.zeros(p.shape[:2], dtype=bool) for p in photos]
    ctrl, ca, cb, inv_ramp, texture, seamless = (np.asarray(a, F32).astype(dt) for a in (ctrl, coef_a, coef_b, inv_ramp, texture, seamless))
    gain = None if gain is None else np.asarray(gain, F32).astype(dt)
    for b, (row, drow) in enumerate(zip(np.asarray(rows).tolist(), np.asarray(drows).tolist())):
        img, y0, x0, y1, x1 = row
        if img < 0 or img >= len(out) or not _active(drow, len(donors)):
            continue
        ph = out[img]
        px = _box_pixels(row, *ph.shape[:2])
        if px is None:
            continue
        r, c = px
        w = weight(edges[b], isoft[b], y1 - y0, x1 - x0)[r - y0, c - x0]
        r, c, w = r[w > 0], c[w > 0], w[w > 0]
        if not len(r):
            continue
        rr, cc = (r - y0).astype(dt), (c - x0).astype(dt)
        mix, ok, _place = mixer(photos, donors, row, drow, ctrl[b], ca[b], cb[b], texture[b], None if gain is None else gain[b], rr, cc)
        if not ok.any():
            continue
        r, c, w, rr, cc, mix = r[ok], c[ok], w[ok], rr[ok], cc[ok], mix[ok]
        with np.errstate(all='ignore'):
            sr = seamless[b] * field(ring[b], diff[b], rr, cc, dt)
            mix = mix + sr
            wy = np.minimum(dt(1), (np.minimum(r - y0, y1 - 1 - r).astype(dt) + dt(0.5)) * inv_ramp[b, 0])
            wx = np.minimum(dt(1), (np.minimum(c - x0, x1 - 1 - c).astype(dt) + dt(0.5)) * inv_ramp[b, 1])
            p = ph[r, c].astype(dt)
            if dt is F32:
                ramp = wy * wx
                a = (ramp * w)[:, None]
                d = mix - p
                mm = a * d
                v = np.fmin(np.fmax(np.rint(p + mm), dt(0)), dt(255))
            else:
                a = (wy * wx * w)[:, None]
                v = np.fmin(np.fmax(np.rint((1 - a) * p + a * mix), 0), 255)
        assert v.dtype == dt
        ph[r, c] = v.astype(np.uint8)
        covered[img][r, c] = True
    return out, covered


def morph_seam_f32(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, inv_ramp, edges, isoft, ring, diff, seamless, gain=None):
    """hull_reference.morph_f32 with mix + seamless * field in the kernel's f32 order -> (new photos, covered)."""
    return _morph_seam(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, inv_ramp, edges, isoft, ring, diff, seamless, gain, F32)


def morph_seam_f64(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, inv_ramp, edges, isoft, ring, diff, seamless, gain=None):
    """hull_reference.morph_f64 with mix + seamless * field in float64 from the f32 ring and diffs widened."""
    return _morph_seam(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, inv_ramp, edges, isoft, ring, diff, seamless, gain, F64)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
# Two photos of 64 x 80 and 50 x 61 (an odd width) and three donor photos; boxes of about 40 x 48 pixels.
#   0, 1   overlap in photo 0
#   2      its box holds the whole of photo 1 with a margin and its hull, grown twice, leaves the box: the side lines bind.  The binding
#          sides lie outside the photo: a pixel ON a binding side lies on the ring's polygon, where the rule gives 0 / 0 and its f32 and
#          f64 forms need not agree (include/imm_seam.h, "What the rule does NOT do")
#   3      its landmarks are moved down until their mean is y = 1.05: their centroid lies below the box, outside the region (flag bit 0), while
#          the hull still reaches into the box
#   4      a NaN landmark: the hull is flagged (and so is the fit)
#   5      its donor photo does not exist: the row is not active
#   6      a plain row in photo 1, under row 2
PHOTOS, DONORS = [(64, 80), (50, 61)], [(40, 44), (31, 29), (36, 50)]
ROWS = [(0, 6, 4, 46, 52), (0, 20, 28, 60, 76), (1, -4, -5, 54, 66), (0, 2, 30, 42, 78), (1, 5, 8, 45, 56), (0, 10, 10, 50, 58),
        (1, 8, 10, 48, 58)]
DONOR_ROWS = [(0, 2, 3, 38, 41), (1, 1, 2, 29, 27), (2, 0, 4, 36, 46), (0, 0, 0, 40, 44), (1, 3, 3, 25, 25), (7, 2, 2, 30, 30),
              (2, 4, 2, 34, 48)]
SIDES_ROW, OUTSIDE_ROW, NAN_ROW, INACTIVE_ROW = 2, 3, 4, 5
GROWS = np.array([1.25, 1.25, 2.0, 1.25, 1.25, 1.25, 1.25], F32)
SEAMLESS = np.array([1.0, 0.6, 1.0, 1.0, 1.0, 1.0, 0.0], F32)
KERNEL_SHAPES, RINGS, FEATHERS, MASK_FEATHER = R.KERNEL_SHAPES, (16, 128), (0.0, 0.125), 0.1
SEED = 11


def kernel_case(K, m, seed=SEED):
    """(photos, rows int32 [n, 5], donors, drows int32 [n, 5], mu_a, mu_b f32 [n, K, 2], shape f32 [n], texture f32 [n], grow f32 [n],
    seamless f32 [n]): smooth photos (the membrane is meant for skin, not for noise), landmarks on morph_reference's jittered grid."""
    from alignment_reference import smooth_photo
    rng = np.random.RandomState(seed + 37 * K)
    rows, drows = np.array(ROWS, dtype=np.int32), np.array(DONOR_ROWS, dtype=np.int32)
    n = len(rows)
    mu_a, mu_b = R.landmarks(K, n, rng)
    for mu in (mu_a, mu_b):                                                   # the centroid at y = 1.05: (1.05 + 1) * H / 2 > H - 1 for H = 40
        mu[OUTSIDE_ROW, :, 0] += F32(1.05) - mu[OUTSIDE_ROW, :, 0].mean(dtype=F64).astype(F32)
    mu_a[NAN_ROW, K // 2, 1] = np.nan
    shape, texture = rng.uniform(0.05, 0.95, n).astype(F32), rng.uniform(0.5, 1.0, n).astype(F32)
    shape[0], texture[0] = 0.0, 1.0                                           # the swap
    photos = [smooth_photo(h, w, seed + i) for i, (h, w) in enumerate(PHOTOS)]
    donors = [(smooth_photo(h, w, seed + 20 + i) * 0.7 + 30 + 10 * i).astype(np.uint8) for i, (h, w) in enumerate(DONORS)]
    return photos, rows, donors, drows, mu_a, mu_b, shape, texture, GROWS.copy(), SEAMLESS.copy()


def fitted_case(K, m, lam=0.0):
    """kernel_case with its blended poses, its f64 fit rounded to f32 and its lines: (case, poses, coef_a, coef_b f32, ctrl f32, edges,
    hull flags)."""
    case = kernel_case(K, m)
    poses = R.blend_f32(case[4], case[5], case[6])
    coef_a, coef_b, ctrl, _flags, _cond = R.fit2_f64(case[4], case[5], poses, m, lam)
    edges, hflags = HR.hull_fit(poses, case[1], case[8])
    return case, poses, coef_a.astype(F32), coef_b.astype(F32), ctrl, edges, hflags


# The flat-photo known answer: a square hull with its sides at half pixels, its corners on the diagonals, so that the ring's samples
# at 45, 135, 225 and 315 degrees are the corners for every B that 8 divides and the ring's polygon IS the hull; every pixel with w > 0
# lies at least half a pixel inside it.
FLAT_SQUARE = [(4.5, 4.5), (4.5, 27.5), (27.5, 27.5), (27.5, 4.5)]


def flat_case():
    """Two flat photos and one row whose four landmarks are FLAT_SQUARE on both sides (the spline is the identity):
    (photo, donor, rows, drows, poses f32 [1, 4, 2])."""
    import colour_reference as CO
    photo, donor = CO.flat_photo(48, 57, (200, 17, 99)), CO.flat_photo(30, 21, (90, 30, 140))
    rows, drows = np.array([(0, 4, 20, 36, 52)], dtype=np.int32), np.array([(0, 3, 2, 25, 18)], dtype=np.int32)
    poses = HR.poses_of(FLAT_SQUARE, 32, 32)[None]
    assert np.array_equal((poses.astype(F64) + 1) * 16, np.array([FLAT_SQUARE])), 'exact in f32'
    return photo, donor, rows, drows, poses
