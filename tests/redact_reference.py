"""The rule of imm_redact_cells_u8 / imm_redact_u8 (include/imm_redact.h) restated in numpy.

grid            (cell, gy, gx) of a box row in Python integers
cells           one row's slice of the cells buffer, u8 [blocks * blocks * 3], in integers: what the kernel must equal byte for byte
cells_all       the whole buffer u8 [n, blocks * blocks * 3]
paste           the paste over copies of the photos, rows applied in row order with a rint after every row (what the kernel's
                ownership and link walks amount to, as in compose_reference): dtype float32 in the kernel's operation order (numpy
                rounds every f32 operation separately), the bytes the kernel must equal; dtype float64 from the formulas (weights
                (1 - t), t on the taps, (1 - a) p + a g), the witness that the f32 order computes what the rule says
and the shared inputs of the kernel tests (tests/test_redact_cpu.py, tests/test_redact_gpu.py)."""
import numpy as np

import hull_reference as HR
from compose_reference import pack, unpack                                  # noqa: F401  (the tests take them from here)
from morph_reference import _sample_f32, _sample_f64
from warp_reference import _box_pixels, inv_ramp                             # noqa: F401

F32 = np.float32
PIXELATE, SMOOTH = 0, 1


def grid(row, blocks):
    """(cell, gy, gx) of a box row (image, y0, x0, y1, x1); (0, 0, 0) for an empty or inverted box."""
    _img, y0, x0, y1, x1 = (int(v) for v in row)
    H, W = y1 - y0, x1 - x0
    if H <= 0 or W <= 0:
        return 0, 0, 0
    cell = max(1, (max(H, W) + blocks - 1) // blocks)
    return cell, (H + cell - 1) // cell, (W + cell - 1) // cell


def active(row, n_images):
    return 0 <= int(row[0]) < n_images and grid(row, 1)[0] > 0


def cells(photo, row, blocks):
    """One row's slice u8 [blocks * blocks * 3]: photo u8 [h, w, 3], or None for a row whose image index is out of range."""
    out = np.zeros(blocks * blocks * 3, np.uint8)
    cell, gy, gx = grid(row, blocks)
    if photo is None or not cell:
        return out
    _img, y0, x0, y1, x1 = (int(v) for v in row)
    h, w = photo.shape[:2]
    H, W = y1 - y0, x1 - x0
    # only the cells that can meet the photo are visited (the others stay 0): a huge box costs what the photo costs
    for i in range(max(0, -y0 // cell), min(gy, (h - y0 + cell - 1) // cell)):
        ra, rb = max(y0 + i * cell, 0), min(y0 + min((i + 1) * cell, H), h)
        if rb <= ra:
            continue
        for j in range(max(0, -x0 // cell), min(gx, (w - x0 + cell - 1) // cell)):
            ca, cb = max(x0 + j * cell, 0), min(x0 + min((j + 1) * cell, W), w)
            if cb <= ca:
                continue
            cnt = (rb - ra) * (cb - ca)
            s = photo[ra:rb, ca:cb].reshape(-1, 3).astype(np.int64).sum(axis=0)
            out[(i * gx + j) * 3:(i * gx + j) * 3 + 3] = [(2 * int(v) + cnt) // (2 * cnt) for v in s]
    return out


def full_grid(row, blocks, sizes):
    """True for an active row every cell of which holds a pixel of its photo (sizes: (h, w) per photo): the rows for which
    consequence (b) of the header holds in the smooth mode as well."""
    if not active(row, len(sizes)):
        return False
    _img, y0, x0, y1, x1 = (int(v) for v in row)
    h, w = sizes[int(row[0])]
    cell, gy, gx = grid(row, blocks)
    return y0 + min(cell, y1 - y0) > 0 and x0 + min(cell, x1 - x0) > 0 and y0 + (gy - 1) * cell < h and x0 + (gx - 1) * cell < w


def cells_all(photos, rows, blocks):
    rows = np.asarray(rows).reshape(-1, 5)
    return np.stack([cells(photos[int(r[0])] if 0 <= int(r[0]) < len(photos) else None, r, blocks) for r in rows])


def weight_at(edges, inv_soft, dy, dx, wide=False):
    """The hull weight of include/imm_hull.h at the box-relative pixels (dy, dx) alone (hull_reference's weight maps span the whole
    box, which a box of side 100 000 does not allow): f32 in the kernel's order, or f64 from the f32 lines widened."""
    ft = np.float64 if wide else F32
    e = np.asarray(edges, F32).astype(ft)
    rr, cc = np.asarray(dy).astype(ft), np.asarray(dx).astype(ft)
    dist = np.full(rr.shape, np.inf, ft)
    with np.errstate(all='ignore'):
        for ny, nx, d in e:
            dist = np.fmin(dist, (ny * rr + nx * cc) + d)
        w = np.fmin(np.fmax(dist * ft(F32(inv_soft)), ft(0)), ft(1))
    assert w.dtype == ft
    return w


def paste(photos, rows, cell_buf, blocks, mode, ramp, edges=None, isoft=None, hull_flags=None, dtype=np.float32):
    """photos: list of u8 [h, w, 3]; rows int [n, 5]; cell_buf u8 [n, blocks * blocks * 3]; ramp f32 [n, 2] (inv_ramp); edges f32
    [n, K, 3], isoft f32 [n] and hull_flags int [n], or None each -> (new photos, per photo the bool mask of the pixels some row
    WROTE: inside the box of an active row and, with the mask, with a weight > 0 or in a flagged row)."""
    wide = dtype == np.float64
    ft = np.float64 if wide else F32
    out = [np.array(p, dtype=np.uint8, copy=True) for p in photos]
    covered = [np.zeros(p.shape[:2], dtype=bool) for p in photos]
    ramp = np.asarray(ramp, F32).astype(ft)
    for b, row in enumerate(np.asarray(rows).reshape(-1, 5).tolist()):
        if not active(row, len(out)):
            continue
        img, y0, x0, y1, x1 = row
        ph = out[img]
        px = _box_pixels(row, *ph.shape[:2])
        if px is None:
            continue
        r, c = px
        cell, gy, gx = grid(row, blocks)
        w = None
        if edges is not None and not int(hull_flags[b]):
            w = weight_at(edges[b], isoft[b], r - y0, c - x0, wide)
            r, c, w = r[w > 0], c[w > 0], w[w > 0]
            if not len(r):
                continue
        means = np.asarray(cell_buf[b][:gy * gx * 3]).reshape(gy, gx, 3)
        dy, dx = (r - y0).astype(np.int64), (c - x0).astype(np.int64)
        with np.errstate(all='ignore'):
            if mode == PIXELATE:
                g = means[dy // cell, dx // cell].astype(ft)
            elif wide:
                g = _sample_f64(means, (dy + 0.5) / cell - 0.5, (dx + 0.5) / cell - 0.5)
            else:
                inv = F32(1.0 / np.float64(cell))
                g = _sample_f32(means, (dy.astype(F32) + F32(0.5)) * inv - F32(0.5), (dx.astype(F32) + F32(0.5)) * inv - F32(0.5))
            wy = np.minimum(ft(1), (np.minimum(r - y0, y1 - 1 - r).astype(ft) + ft(0.5)) * ramp[b, 0])
            wx = np.minimum(ft(1), (np.minimum(c - x0, x1 - 1 - c).astype(ft) + ft(0.5)) * ramp[b, 1])
            a = wy * wx
            if edges is not None:
                a = a * (ft(1) if w is None else w)
            a = a[:, None]
            p = ph[r, c].astype(ft)
            if wide:
                v = np.fmin(np.fmax(np.rint((1 - a) * p + a * g), 0), 255)
            else:
                d = g - p
                mm = a * d
                v = np.fmin(np.fmax(np.rint(p + mm), F32(0)), F32(255))
        assert v.dtype == ft and a.dtype == ft and g.dtype == ft
        ph[r, c] = v.astype(np.uint8)
        covered[img][r, c] = True
    return out, covered


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
BLOCKS = (1, 2, 7, 8, 64)
FEATHERS = (0.0, 0.125)
SIZES = ((37, 53), (64, 80), (1, 1))
# photo 0 is 37 x 53, photo 1 is 64 x 80, photo 2 is 1 x 1
ROWS = [
    (0, 5, 7, 30, 40),                        # inside
    (1, 30, 30, 55, 60),                      # three overlapping rows of photo 1 ...
    (1, 40, 40, 63, 75),
    (0, 10, 10, 25, 25),                      # ... with one of another photo between them (it overlaps row 0 as well)
    (1, 35, 20, 50, 70),
    (0, -6, 10, 12, 30),                      # cut by the top edge
    (0, 25, 10, 45, 30),                      # the bottom edge
    (0, 8, -9, 20, 11),                       # the left edge
    (0, 8, 40, 22, 60),                       # the right edge
    (0, 50, 60, 70, 90),                      # wholly outside
    (1, 10, 10, 10, 30),                      # empty
    (1, 30, 10, 20, 5),                       # inverted
    (1, 3, 4, 4, 5),                          # 1 x 1
    (1, 20, -5, 25, 85),                      # 5 x 90, elongated
    (0, 18 - 50000, 26 - 50000, 18 + 50000, 26 + 50000),      # side 100 000 around photo 0
    (-1, 0, 0, 10, 10),                       # image index -1
    (3, 0, 0, 10, 10),                        # image index n_images
    (2, 0, 0, 1, 1),                          # the 1 x 1 photo
    (2, -3, -3, 4, 4),
]


def photos_of(seed=7):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES]


def case_rows(n, seed=11):
    """int32 [n, 5]: n = 1: the inside box; n = 3: the first three of ROWS (two overlap); else ROWS, then random boxes over the three
    photos, some reaching outside."""
    rows = list(ROWS[:n])
    rng = np.random.RandomState(seed + n)
    while len(rows) < n:
        img = int(rng.randint(0, 3))
        h, w = SIZES[img]
        y0, x0 = int(rng.randint(-8, h)), int(rng.randint(-8, w))
        rows.append((img, y0, x0, y0 + int(rng.randint(1, 40)), x0 + int(rng.randint(1, 40))))
    return np.array(rows, np.int32)


def hull_case(rows, K=7, seed=5):
    """Edges from hull_reference on random clouds for `rows`, with a row of flags 1 (NaN landmark) and a row of flags 2 (collinear
    points) among the active rows -> (poses f32 [n, K, 2], edges f32 [n, K, 3], flags int32 [n], inv_soft f32 [n], the two rows)."""
    rows = np.asarray(rows).reshape(-1, 5)
    n = len(rows)
    rng = np.random.RandomState(seed + n)
    poses = rng.uniform(-0.8, 0.8, (n, K, 2)).astype(F32)
    act = [b for b in range(n) if active(rows[b], len(SIZES)) and _box_pixels(rows[b].tolist(), *SIZES[rows[b][0]]) is not None]
    nan_row, flat_row = act[0], act[min(1, len(act) - 1)]
    if flat_row != nan_row:
        t = np.linspace(-0.5, 0.5, K, dtype=F32)
        poses[flat_row] = np.stack([t, t], axis=1)
    poses[nan_row, K // 2, 0] = np.nan
    edges, flags = HR.hull_fit(poses, rows, np.full(n, 1.25, F32))
    return poses, edges, flags, HR.inv_soft(rows, 0.1), (nan_row, flat_row)
