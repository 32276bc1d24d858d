"""The rule of imm_annotate_points / imm_annotate_u8 (include/imm_annotate.h) restated in numpy.

points          the landmarks in photo pixels, f64 from the inputs widened, rounded once to f32: what the kernel must equal bit for bit
annotate        the paste over copies of the photos, rows applied in row order with a rint after every blend (what the kernel's
                ownership and link walks amount to, as in redact_reference): float32 in the kernel's operation order (numpy rounds every
                f32 operation separately), the bytes the kernel must equal
and the shared inputs of the kernel tests (tests/test_annotate_cpu.py, tests/test_annotate_gpu.py).  Only the pixels near a mark are
visited for it: a window that holds every pixel the rule's own comparison |dy|, |dx| <= R + 2 can accept, inside which that comparison
is made in f32 as the kernel makes it."""
import math

import numpy as np

from redact_reference import pack, unpack, photos_of, case_rows, SIZES, ROWS      # noqa: F401  (the tests take them from here)

F32 = np.float32
POINTS, BOX, HULL, LABEL = 1, 2, 4, 8
ALL = POINTS | BOX | HULL | LABEL
WHITE = np.array([255, 255, 255], F32)
PALETTE = np.array([(40, 220, 60), (235, 30, 30), (255, 150, 0), (250, 230, 20)], np.uint8)        # ok, lost, outside, unsure
SHAPES = 'vosd^x+'
FONT = ('01110 10001 10011 10101 11001 10001 01110', '00100 01100 00100 00100 00100 00100 01110', '01110 10001 00001 00010 00100 01000 11111',
        '11111 00010 00100 00010 00001 10001 01110', '00010 00110 01010 10010 11111 00010 00010', '11111 10000 11110 00001 00001 10001 01110',
        '00110 01000 10000 11110 10001 10001 01110', '11111 00001 00010 00100 01000 01000 01000', '01110 10001 10001 01110 10001 10001 01110',
        '01110 10001 10001 01111 00001 00010 01100')
FONT_BITS = np.array([[[ch == '1' for ch in line] for line in d.split()] for d in FONT])          # bool [10, 7, 5]


def points(mu, rows):
    """mu f32 [n, K, 2], rows int [n, 5] -> f32 [n, K, 2]: y0 + (mu + 1) * (0.5 * H) in f64; a value that is not finite keeps its bits."""
    mu = np.asarray(mu, F32)
    rows = np.asarray(rows).reshape(-1, 5).astype(np.float64)
    origin = rows[:, None, 1:3]
    side = rows[:, None, 3:5] - rows[:, None, 1:3]
    with np.errstate(all='ignore'):
        half = 0.5 * side
        a = mu.astype(np.float64) + 1.0
        m = a * half
        out = (origin + m).astype(F32)
    return np.where(np.isfinite(mu), out, mu)


def colour_index(s, P):
    s = int(s) & 0xFFFFFFFF
    if s == 0:
        return 0
    return min(1 + ((s & -s).bit_length() - 1), P - 1)


def clamp(x):
    with np.errstate(all='ignore'):
        return np.fmin(np.fmax(x, F32(0)), F32(1))


def blend(v, sel, g, a):
    """v f32 [h, w, 3] <- rint(v + a * (g - v)) clamped, at the pixels sel (bool [h, w]); a f32 [h, w] or a scalar."""
    if not sel.any():
        return
    p = v[sel]
    a = F32(a) if np.isscalar(a) else np.broadcast_to(a, sel.shape)[sel][:, None]
    with np.errstate(all='ignore'):
        d = np.asarray(g, F32) - p
        m = a * d
        out = np.fmin(np.fmax(np.rint(p + m), F32(0)), F32(255))
    assert out.dtype == F32
    v[sel] = out


def shape_s(shape, dy, dx, ay, ax, R, inv2R, h):
    """The inside-ness of the header's table; dy [h, 1] and dx [1, w] broadcast."""
    c1, c2 = F32(0.70710677), F32(0.8944272)
    with np.errstate(all='ignore'):
        if shape == 0:
            return np.fmin(dy + R, ((R - dy) * F32(0.5) - ax) * c2)
        if shape == 1:
            return (R * R - (dy * dy + dx * dx)) * inv2R
        if shape == 2:
            return R - np.fmax(ay, ax)
        if shape == 3:
            return (R - (ay + ax)) * c1
        if shape == 4:
            ny = -dy
            return np.fmin(ny + R, ((R - ny) * F32(0.5) - ax) * c2)
        if shape == 5:
            return np.fmin(h - np.fmin(np.abs(dy - dx), np.abs(dy + dx)) * c1, R - np.fmax(ay, ax))
        if shape == 6:
            return np.fmin(h - np.fmin(ay, ax), R - np.fmax(ay, ax))
    return np.full(np.broadcast(dy, dx).shape, -np.inf, F32)


def _window(m, lim, lo, hi):
    """The integers of [lo, hi) within lim + 1 of m: every pixel coordinate the f32 comparison can accept, and a few more."""
    m, lim = float(m), float(lim)
    if not math.isfinite(m) or not math.isfinite(lim):
        return lo, lo
    return max(lo, int(math.floor(m - lim - 1))), min(hi, int(math.ceil(m + lim + 1)) + 1)


def annotate(photos, rows, bits, thickness, pad, scale, palette=PALETTE, marks=None, gstyle=None, mstyle=None, edges=None, status=None,
             labels=None):
    """photos: list of u8 [h, w, 3]; rows int [n, 5]; marks f32 [G, n, K, 2], gstyle f32 [G, 4], mstyle u8 [K, 4], edges f32 [n, K, 3],
    status int [n], labels int [n], or None each -> (new photos, per photo the bool mask of the pixels inside the extent of an active
    row, per photo the bool mask of the pixels some primitive blended)."""
    out = [np.array(p, dtype=np.uint8, copy=True) for p in photos]
    covered = [np.zeros(p.shape[:2], dtype=bool) for p in photos]
    drawn = [np.zeros(p.shape[:2], dtype=bool) for p in photos]
    palette = np.asarray(palette, np.uint8)
    thickness, pad, scale = int(thickness), int(pad), int(scale)
    for b, row in enumerate(np.asarray(rows).reshape(-1, 5).tolist()):
        img, y0, x0, y1, x1 = row
        if not 0 <= img < len(out) or y1 - y0 <= 0 or x1 - x0 <= 0:
            continue
        ph = out[img]
        h, w = ph.shape[:2]
        ey0, ex0, ey1, ex1 = max(y0 - pad, 0), max(x0 - pad, 0), min(y1 + pad, h), min(x1 + pad, w)
        if ey1 <= ey0 or ex1 <= ex0:
            continue
        covered[img][ey0:ey1, ex0:ex1] = True
        v = ph[ey0:ey1, ex0:ex1].astype(F32)
        hit = np.zeros(v.shape[:2], dtype=bool)
        r, c = np.arange(ey0, ey1, dtype=np.int64)[:, None], np.arange(ex0, ex1, dtype=np.int64)[None, :]
        in_box = (r >= y0) & (r < y1) & (c >= x0) & (c < x1)
        s = 0 if status is None else int(status[b])
        lost = bool(s & 1)
        col = palette[colour_index(s, len(palette))].astype(F32)
        if bits & BOX:
            ring = in_box & (np.minimum(np.minimum(r - y0, y1 - 1 - r), np.minimum(c - x0, x1 - 1 - c)) < thickness)
            blend(v, ring, col, 1)
            hit |= ring
        if bits & HULL and not lost:
            rr, cc = (r - y0).astype(F32), (c - x0).astype(F32)
            dist = np.full(np.broadcast(rr, cc).shape, np.inf, F32)
            with np.errstate(all='ignore'):
                for ny, nx, d in np.asarray(edges[b], F32):
                    dist = np.fmin(dist, (ny * rr + nx * cc) + d)
                half = F32(0.5) * F32(thickness) + F32(0.5)
                a = clamp(half - np.abs(dist))
            assert a.dtype == F32
            blend(v, a > 0, col, a)
            hit |= a > 0
        if bits & POINTS and not lost:
            G, K = len(marks), marks.shape[2]
            for g in range(G):
                R, inv2R, hs, alpha = (F32(t) for t in gstyle[g])
                with np.errstate(all='ignore'):
                    lim = R + F32(2)
                for k in range(K):
                    my, mx = F32(marks[g, b, k, 0]), F32(marks[g, b, k, 1])
                    ra, rb = _window(my, lim, ey0, ey1)
                    ca, cb = _window(mx, lim, ex0, ex1)
                    if rb <= ra or cb <= ca:
                        continue
                    with np.errstate(all='ignore'):
                        dy = np.arange(ra, rb, dtype=np.int64).astype(F32)[:, None] - my
                        dx = np.arange(ca, cb, dtype=np.int64).astype(F32)[None, :] - mx
                        ay, ax = np.abs(dy), np.abs(dx)
                        ok = (ay <= lim) & (ax <= lim)
                        if not ok.any():
                            continue
                        trail = g < G - 1
                        sv = shape_s(1 if trail else int(mstyle[k, 3]), dy, dx, ay, ax, R, inv2R, hs)
                        aw = alpha * clamp(sv + F32(1.5))
                        ac = alpha * clamp(sv + F32(0.5))
                    assert sv.dtype == F32 and ac.dtype == F32
                    sub, sub_hit = v[ra - ey0:rb - ey0, ca - ex0:cb - ex0], hit[ra - ey0:rb - ey0, ca - ex0:cb - ex0]
                    if not trail:
                        blend(sub, ok & (aw > 0), WHITE, aw)
                        sub_hit |= ok & (aw > 0)
                    blend(sub, ok & (ac > 0), mstyle[k, :3].astype(F32), ac)
                    sub_hit |= ok & (ac > 0)
        L = -1 if not bits & LABEL else int(labels[b])
        if 0 <= L <= 9999:
            digits = [int(ch) for ch in str(L)]
            nd = len(digits)
            u, t = r - y0 - thickness, c - x0 - thickness
            rect = in_box & (u >= 0) & (u < 9 * scale) & (t >= 0) & (t < (6 * nd + 1) * scale)
            fr, tc = u // scale - 1, t // scale - 1
            di, fc = tc // 6, tc - 6 * (tc // 6)
            on = np.zeros(rect.shape, dtype=bool)
            ok = rect & (fr >= 0) & (fr < 7) & (tc >= 0) & (fc < 5)
            if ok.any():
                rr_i, cc_i = np.nonzero(ok)
                dg = np.array(digits)[di[0, cc_i]]
                on[rr_i, cc_i] = FONT_BITS[dg, fr[rr_i, 0], fc[0, cc_i]]
            blend(v, rect & on, WHITE, 1)
            blend(v, rect & ~on, col, 1)
            hit |= rect
        ph[ey0:ey1, ex0:ex1] = v.astype(np.uint8)
        drawn[img][ey0:ey1, ex0:ex1] |= hit
    return out, covered, drawn


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def mark_styles(K):
    """u8 [K, 4]: 8 colours x 7 shapes, colour cycling fastest, starting again past 56 (the host's table, restated)."""
    colours = [(27, 158, 119), (217, 95, 2), (117, 112, 179), (231, 41, 138), (102, 166, 30), (230, 171, 2), (166, 118, 29), (102, 102, 102)]
    return np.array([colours[(k % 56) % 8] + ((k % 56) // 8,) for k in range(K)], np.uint8)


def group_styles(size, G, alpha=1.0):
    out = np.empty((G, 4), np.float64)
    for g in range(G):
        last = g == G - 1
        R = size if last else max(0.5, 0.5 * size)
        out[g] = (R, 1.0 / (2.0 * R), max(0.5, 0.25 * size), alpha if last else alpha * 0.7 * (g + 1) / G)
    return out.astype(F32)


def case_marks(rows, K, G, pad, seed=3):
    """f32 [G, n, K, 2] in photo pixels: per row marks at pixel centres, at fractional places, on the extent's edge, outside it and at
    NaN (and one at inf), the rest spread over the extent."""
    rows = np.asarray(rows).reshape(-1, 5)
    n = len(rows)
    rng = np.random.RandomState(seed + 7 * n + K + G)
    m = np.empty((G, n, K, 2), F32)
    for b, (img, y0, x0, y1, x1) in enumerate(rows.tolist()):
        h, w = SIZES[img] if 0 <= img < len(SIZES) else (10, 10)
        # (a huge box is sampled where its photo is)
        a0, a1, b0, b1 = max(y0 - pad, -4), min(y1 + pad, h + 4), max(x0 - pad, -4), min(x1 + pad, w + 4)
        if a1 <= a0 or b1 <= b0:
            a0, a1, b0, b1 = y0, y0 + 1, x0, x0 + 1
        for g in range(G):
            pts = np.stack([rng.uniform(a0, a1, K), rng.uniform(b0, b1, K)], axis=1)
            special = [(round((a0 + a1) / 2), round((b0 + b1) / 2)),            # a pixel centre
                       (a0 + 0.5, b0 + 0.25),                                      # fractional, at the extent's corner
                       (float(y0 - pad), float(x0 + 1)),                           # on the extent's edge
                       (y0 - pad - 40.0, x0 - 3.0),                                # outside
                       (np.nan, (b0 + b1) / 2), ((a0 + a1) / 2, np.inf)]
            for i, p in enumerate(special):
                if K > 1 and (i + b + g) % K != 0 or K == 1 and (b + g) % 7 == i:
                    pts[(i + b + g) % K] = p
            if b % 3 == 0:
                pts[:K // 2] = np.round(pts[:K // 2])                              # integer places
            m[g, b] = pts.astype(F32)
    return m


def case_status(n):
    """int32 [n]: 0 mostly; bits 0, 1, 2 alone, mixed (3, 6), a high bit (clamped to the last colour) and a negative value."""
    s = np.zeros(n, np.int32)
    for i, v in enumerate((0, 1, 2, 4, 0, 3, 6, 0, 1 << 20, -2 ** 31, 0, 5)):
        if i < n:
            s[i] = v
    if n > 12:
        s[12:] = np.random.RandomState(n).choice([0, 0, 0, 1, 2, 4], n - 12)
    return s


def case_labels(n):
    """int32 [n]: the row's number, with 10, 123, 9999, 10000 and -1 among them."""
    lab = np.arange(n, dtype=np.int32)
    for i, v in ((1, 10), (2, 123), (3, 9999), (4, 10000), (5, -1), (6, 7), (7, 4086)):
        if i < n:
            lab[i] = v
    return lab
