"""The rule of imm_hull_fit / imm_morph_hull_u8 (include/imm_hull.h) restated in numpy.

hull_fit        (edges f32 [n, K, 3], flags int32 [n]) in float64 in the kernel's operation order (numpy rounds every operation
                separately; division and sqrt are correctly rounded on both sides): what the kernel must equal bit for bit
hull_exact      the same rule in exact rational arithmetic (Python integers over a common denominator) on the same f32 inputs: which
                slots have a winner, and whether any point lies strictly inside a winner's line
weight_f32      the weight over a row's box in the kernel's f32 order; weight_f64 the same from the f32 lines widened
inside_count    the lattice points strictly inside a polygon, in integers (a known answer that needs none of the above)
morph_f64 / morph_f32   colour_reference's two restatements (gain optional) with the weight: a pixel with !(w > 0) is left alone, every
                other is blended by the ramp times w
and the shared inputs of the kernel tests (tests/test_hull_cpu.py, tests/test_hull_gpu.py)."""
from fractions import Fraction
from math import lcm

import numpy as np

import morph_reference as R
from morph_reference import _active, _sample_f32, _sample_f64
from warp_reference import U, _box_pixels

F32 = np.float32
NO_HULL = np.array([0.0, 0.0, -np.inf], F32)          # every slot of a flagged row
NO_WINNER = np.array([0.0, 0.0, np.inf], F32)         # a slot without a winner


def hull_fit(poses, rows, grow):
    """poses f32 [n, K, 2], rows int [n, 5], grow f32 [n] -> (edges f32 [n, K, 3], flags int32 [n]) in the header's operation order."""
    f64 = np.float64
    p = np.asarray(poses, F32).astype(f64)
    n, K = p.shape[:2]
    rows, grow = np.asarray(rows).reshape(-1, 5), np.asarray(grow, F32).astype(f64)
    edges, flags = np.zeros((n, K, 3), F32), np.zeros(n, np.int32)
    for b in range(n):
        H, W = int(rows[b, 3]) - int(rows[b, 1]), int(rows[b, 4]) - int(rows[b, 2])
        g = grow[b]
        with np.errstate(all='ignore'):
            vy, vx = (p[b, :, 0] + 1.0) * (0.5 * f64(H)), (p[b, :, 1] + 1.0) * (0.5 * f64(W))
            sy, sx = vy[0], vx[0]
            for i in range(1, K):                                              # in index order
                sy, sx = sy + vy[i], sx + vx[i]
            cy, cx = sy / f64(K), sx / f64(K)
            vy, vx = cy + g * (vy - cy), cx + g * (vx - cx)
            ey, ex = vy[None, :] - vy[:, None], vx[None, :] - vx[:, None]      # [i, j] = v_j - v_i
            s = ey[:, :, None] * ex[:, None, :] - ex[:, :, None] * ey[:, None, :]      # [i, j, k]
            cand = ~((ey == 0.0) & (ex == 0.0)) & (s >= 0.0).all(axis=2)
            inner = cand & (s > 0.0).any(axis=2)
            l2 = ey * ey + ex * ex
            win = np.argmax(np.where(cand, l2, -1.0), axis=1)                  # the first of the largest: ties go to the lowest j
            has = cand.any(axis=1)
            i = np.arange(K)
            wy, wx, length = ey[i, win], ex[i, win], np.sqrt(l2[i, win])
            ny, nx = -wx / length, wy / length
            d = -(ny * vy + nx * vx)
            line = np.stack([ny, nx, d], axis=1).astype(F32)
        line[~has] = NO_WINNER
        bad = H <= 0 or W <= 0 or not np.isfinite(g) or not np.isfinite(p[b]).all()
        flat = int(has.sum()) < 3 or not inner[i, win][has].any()
        flags[b] = int(bad) | 2 * int(flat)
        edges[b] = NO_HULL if flags[b] else line
    return edges, flags


def hull_exact(pose, row, grow):
    """One row in exact arithmetic: pose f32 [K, 2] (finite), row (image, y0, x0, y1, x1), grow f32 -> (bool [K]: slot i has a winner,
    bool: some point lies strictly inside some line between two of the points that has every point on its inner side)."""
    K = len(pose)
    H, W = int(row[3]) - int(row[1]), int(row[4]) - int(row[2])
    g = Fraction(float(F32(grow)))
    vy = [(Fraction(float(F32(y))) + 1) * Fraction(H, 2) for y in np.asarray(pose)[:, 0]]
    vx = [(Fraction(float(F32(x))) + 1) * Fraction(W, 2) for x in np.asarray(pose)[:, 1]]
    cy, cx = sum(vy) / K, sum(vx) / K
    vy, vx = [cy + g * (v - cy) for v in vy], [cx + g * (v - cx) for v in vx]
    den = lcm(*[v.denominator for v in vy + vx])
    Y, X = np.array([int(v * den) for v in vy], dtype=object), np.array([int(v * den) for v in vx], dtype=object)
    ey, ex = Y[None, :] - Y[:, None], X[None, :] - X[:, None]
    s = ey[:, :, None] * ex[:, None, :] - ex[:, :, None] * ey[:, None, :]
    cand = ~((ey == 0) & (ex == 0)) & (s >= 0).all(axis=2)
    return cand.any(axis=1), bool((cand & (s > 0).any(axis=2)).any())


def weight_f32(edges, inv_soft, H, W):
    """edges f32 [K, 3] -> f32 [H, W] in the kernel's order."""
    e = np.asarray(edges, F32)
    rr, cc = np.arange(max(H, 0), dtype=F32)[:, None], np.arange(max(W, 0), dtype=F32)[None, :]
    dist = np.full((rr.shape[0], cc.shape[1]), np.inf, F32)
    with np.errstate(all='ignore'):
        for ny, nx, d in e:
            dist = np.fmin(dist, (ny * rr + nx * cc) + d)
        w = np.fmin(np.fmax(dist * F32(inv_soft), F32(0)), F32(1))
    assert w.dtype == F32
    return w


def weight_f64(edges, inv_soft, H, W):
    """The same in float64 from the f32 lines and inv_soft widened."""
    e = np.asarray(edges, F32).astype(np.float64)
    rr, cc = np.arange(max(H, 0), dtype=np.float64)[:, None], np.arange(max(W, 0), dtype=np.float64)[None, :]
    dist = np.full((rr.shape[0], cc.shape[1]), np.inf)
    with np.errstate(all='ignore'):
        for ny, nx, d in e:
            dist = np.fmin(dist, ny * rr + nx * cc + d)
        return np.fmin(np.fmax(dist * np.float64(F32(inv_soft)), 0.0), 1.0)


def inside_count(poly, H, W):
    """bool [H, W]: the lattice points (r, c) of [0, H) x [0, W) strictly inside the convex polygon poly (integer (y, x) vertices in
    order, either way round), in integers."""
    r, c = np.arange(H, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    cross = [(by - ay) * (c - ax) - (bx - ax) * (r - ay) for (ay, ax), (by, bx) in zip(poly, poly[1:] + poly[:1])]
    return np.all([x > 0 for x in cross], axis=0) | np.all([x < 0 for x in cross], axis=0)


def inv_soft(rows, mask_feather):
    """(float)(1 / max(1, mask_feather * min(H, W))), in f64 from the f32 mask_feather widened -> f32 [n]."""
    rows = np.asarray(rows).reshape(-1, 5)
    side = np.minimum(rows[:, 3].astype(np.int64) - rows[:, 1], rows[:, 4].astype(np.int64) - rows[:, 2]).astype(np.float64)
    mf = np.broadcast_to(np.asarray(mask_feather, F32), (len(rows),)).astype(np.float64)
    return (1.0 / np.maximum(1.0, mf * side)).astype(F32)


def morph_f64(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, inv_ramp, edges, isoft, gain=None):
    """colour_reference.morph_f64 (gain None: morph_reference.morph_f64) with the weight in float64 -> (new photos, per photo the bool
    mask of the pixels some row WROTE: w > 0 and all four source coordinates finite)."""
    out = [np.array(p, dtype=np.uint8, copy=True) for p in photos]
    covered = [np.zeros(p.shape[:2], dtype=bool) for p in photos]
    ctrl, coef_a, coef_b, inv_ramp, texture = (np.asarray(a, dtype=np.float64) for a in (ctrl, coef_a, coef_b, inv_ramp, texture))
    gain = None if gain is None else np.asarray(gain, dtype=F32).astype(np.float64)
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
        w = weight_f64(edges[b], isoft[b], y1 - y0, x1 - x0)[r - y0, c - x0]
        r, c, w = r[w > 0], c[w > 0], w[w > 0]
        if not len(r):
            continue
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
        r, c, w = r[ok], c[ok], w[ok]
        gA, gB = _sample_f64(src, ay[ok], ax[ok]), _sample_f64(don, by[ok], bx[ok])
        with np.errstate(all='ignore'):
            if gain is not None:
                gB = gB * gain[b, :, 0][None, :] + gain[b, :, 1][None, :]
            mix = (1.0 - texture[b]) * gA + texture[b] * gB
            wy = np.minimum(1.0, (np.minimum(r - y0, y1 - 1 - r) + 0.5) * inv_ramp[b, 0])
            wx = np.minimum(1.0, (np.minimum(c - x0, x1 - 1 - c) + 0.5) * inv_ramp[b, 1])
            a = (wy * wx * w)[:, None]
            p = ph[r, c].astype(np.float64)
            ph[r, c] = np.fmin(np.fmax(np.rint((1 - a) * p + a * mix), 0), 255).astype(np.uint8)
        covered[img][r, c] = True
    return out, covered


def morph_f32(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, inv_ramp, edges, isoft, gain=None):
    """colour_reference.morph_f32 (gain None: morph_reference.morph_f32) with the kernel's weight: w in f32 in the rule's order, a pixel
    with !(w > 0) left alone before anything else, the blend weight ramp * w, one rounded product."""
    f32 = F32
    out = [np.array(p, dtype=np.uint8, copy=True) for p in photos]
    covered = [np.zeros(p.shape[:2], dtype=bool) for p in photos]
    ctrl, ca, cb, inv_ramp, texture = (np.asarray(a, dtype=f32) for a in (ctrl, coef_a, coef_b, inv_ramp, texture))
    gain = None if gain is None else np.asarray(gain, dtype=f32)
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
        w = weight_f32(edges[b], isoft[b], y1 - y0, x1 - x0)[r - y0, c - x0]
        r, c, w = r[w > 0], c[w > 0], w[w > 0]
        if not len(r):
            continue
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
        r, c, w = r[ok], c[ok], w[ok]
        gA, gB = _sample_f32(src, ay[ok], ax[ok]), _sample_f32(don, by[ok], bx[ok])
        with np.errstate(all='ignore'):
            if gain is not None:
                sc = gB * gain[b, :, 0][None, :]
                gB = sc + gain[b, :, 1][None, :]
            e = gB - gA
            te = texture[b] * e
            mix = gA + te
            wy = np.minimum(f32(1), (np.minimum(r - y0, y1 - 1 - r).astype(f32) + f32(0.5)) * inv_ramp[b, 0])
            wx = np.minimum(f32(1), (np.minimum(c - x0, x1 - 1 - c).astype(f32) + f32(0.5)) * inv_ramp[b, 1])
            ramp = wy * wx
            a = (ramp * w)[:, None]
            p = ph[r, c].astype(f32)
            d = mix - p
            mm = a * d
            v = np.fmin(np.fmax(np.rint(p + mm), f32(0)), f32(255))
        assert v.dtype == f32 and a.dtype == f32
        ph[r, c] = v.astype(np.uint8)
        covered[img][r, c] = True
    return out, covered


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
GROW, MASK_FEATHERS = 1.25, (0.1, 0.25)


def poses_of(points, H, W):
    """Box-relative pixel points (y, x) -> f32 poses in the box frame: p = v * 2 / side - 1 (exact for the small integers and power-of-two
    sides of the hand-made cases)."""
    pts = np.asarray(points, np.float64)
    return np.stack([pts[:, 0] * 2.0 / H - 1.0, pts[:, 1] * 2.0 / W - 1.0], axis=1).astype(F32)


SQUARE = [(4, 4), (4, 12), (12, 12), (12, 4)]
# (name, box-relative points, (H, W), flags expected at grow = 1)
CASES = [
    ('triangle', [(2, 3), (13, 5), (6, 14)], (16, 16), 0),
    ('square with an interior point', SQUARE + [(8, 8)], (16, 16), 0),
    ('three collinear points on an edge', SQUARE + [(4, 6), (4, 8), (4, 10)], (16, 16), 0),
    ('duplicated points', SQUARE + SQUARE[1:3] + [(4, 4)], (16, 16), 0),
    ('all points collinear', [(2, 2), (4, 4), (6, 6), (12, 12)], (16, 16), 2),
    ('all points identical', [(5, 7)] * 4, (16, 16), 2),
    ('K = 1', [(5, 7)], (16, 16), 2),
    ('a non-square box', [(2, 3), (13, 5), (15, 20), (6, 21), (8, 10)], (17, 23), 0),
]


def case_inputs(points, hw, grow=1.0, corner=(3, 5)):
    """(poses f32 [1, K, 2], rows int32 [1, 5], grow f32 [1]) of one hand-made case."""
    H, W = hw
    return poses_of(points, H, W)[None], np.array([(0, corner[0], corner[1], corner[0] + H, corner[1] + W)], np.int32), np.array([grow], F32)


def kernel_poses(K, m):
    """morph_reference.kernel_case with its blended poses: (case, poses f32 [n, K, 2])."""
    case = R.kernel_case(K, m)
    return case, R.blend_f32(case[4], case[5], case[6])


def fit_rows(n, K, seed=3):
    """The GPU test's rows of imm_hull_fit: the hand-made cases where they fit K (else points on a jittered ring or a cloud), then NaN
    and infinite poses, grows 0.5, 1, 1.5 and NaN, empty and inverted boxes, boxes with sides beyond 16 bits
    -> (poses f32 [n, K, 2], rows int32 [n, 5], grow f32 [n])."""
    rng = np.random.RandomState(seed + 100 * n + K)
    poses = rng.uniform(-0.9, 0.9, (n, K, 2)).astype(F32)
    rows = np.zeros((n, 5), np.int32)
    grow = np.array([(0.5, 1.0, 1.5, 1.25)[b % 4] for b in range(n)], F32)
    for b in range(n):
        y0, x0 = int(rng.randint(-20, 50)), int(rng.randint(-20, 50))
        rows[b] = (b % 3, y0, x0, y0 + int(rng.randint(1, 70)), x0 + int(rng.randint(1, 70)))
    b = 0
    for _name, pts, hw, _f in [('the square', SQUARE, (16, 16), 0)] + CASES:
        if len(pts) == K and b < n:
            poses[b], rows[b], grow[b] = poses_of(pts, *hw), (0, 3, 5, 3 + hw[0], 5 + hw[1]), 1.0
            b += 1
    special = [('nan', None), ('inf', None), ('-inf', None), ('grow nan', None), ('empty', (1, 10, 10, 10, 30)), ('inverted', (1, 30, 10, 20, 5)),
               ('wide', (0, -40000, -70000, 60000, 80000)), ('widest', (2, -2147483648, -2147483648, 2147483647, 2147483647)),
               ('grow inf', None)]
    for idx, (what, box) in enumerate(special):                               # from the last row backwards; row 0 stays a plain one
        b, first = n - 1 - idx, max(b if idx == 0 else first, 1)
        if b < first:
            break
        if what in ('nan', 'inf', '-inf'):
            poses[b, K // 2, b % 2] = float(what)
        elif what.startswith('grow'):
            grow[b] = float(what.split()[1])
        else:
            rows[b] = box
    return poses, rows, grow
