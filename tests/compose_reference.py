"""The pixel rule of imm_compose_u8 (include/imm_compose.h) restated in numpy, twice: compose_f32 in float32 in the kernel's operation
order (numpy rounds every f32 operation separately, as the kernel's unfused arithmetic does), and compose_f64 in float64 from the
formulas, order-free.  Both apply the rows in row order and round to u8 after every row.  Also the shared inputs of the kernel tests
(tests/test_compose_cpu.py, tests/test_compose_gpu.py) and the packing of photos into the buffer the kernel reads."""
import numpy as np

S_KERNEL = 16


def _clip_box(box, h, w):
    y0, x0, y1, x1 = box
    return np.arange(max(y0, 0), min(y1, h)), np.arange(max(x0, 0), min(x1, w))


def compose_f32(photos, rows, faces, inv_ramp, S):
    """photos: list of u8 [h, w, 3]; rows int [n, 5]; faces f32 [n, S, S, >= 3]; inv_ramp f32 [n, 2] -> new list of u8 photos."""
    f32 = np.float32
    out = [np.array(p, dtype=np.uint8, copy=True) for p in photos]
    faces = np.asarray(faces, dtype=f32)
    inv_ramp = np.asarray(inv_ramp, dtype=f32)
    for b, (img, y0, x0, y1, x1) in enumerate(np.asarray(rows).tolist()):
        ph = out[img]
        r, c = _clip_box((y0, x0, y1, x1), ph.shape[0], ph.shape[1])
        if not len(r) or not len(c):
            continue
        ih, iw = y1 - y0, x1 - x0
        sy = f32(np.float64(S - 1) / np.float64(ih - 1)) if ih > 1 else f32(0)
        sx = f32(np.float64(S - 1) / np.float64(iw - 1)) if iw > 1 else f32(0)
        fy, fx = (r - y0).astype(f32) * sy, (c - x0).astype(f32) * sx
        yl, xl = np.minimum(np.floor(fy).astype(np.int64), S - 1), np.minimum(np.floor(fx).astype(np.int64), S - 1)
        yh, xh = np.minimum(yl + 1, S - 1), np.minimum(xl + 1, S - 1)
        ty, tx = (fy - yl.astype(f32))[:, None, None], (fx - xl.astype(f32))[None, :, None]
        f = faces[b, :, :, :3]
        tl, tr, bl, br = f[yl][:, xl], f[yl][:, xh], f[yh][:, xl], f[yh][:, xh]
        top = tl + (tr - tl) * tx
        bot = bl + (br - bl) * tx
        g = top + (bot - top) * ty
        g = np.minimum(np.maximum(g, f32(0)), f32(255))
        wy = np.minimum(f32(1), (np.minimum(r - y0, y1 - 1 - r).astype(f32) + f32(0.5)) * inv_ramp[b, 0])
        wx = np.minimum(f32(1), (np.minimum(c - x0, x1 - 1 - c).astype(f32) + f32(0.5)) * inv_ramp[b, 1])
        a = (wy[:, None] * wx[None, :])[:, :, None]
        p = ph[r[0]:r[-1] + 1, c[0]:c[-1] + 1].astype(f32)
        d = g - p
        m = a * d
        v = np.rint(p + m)
        assert v.dtype == f32 and v.min() >= 0 and v.max() <= 255
        ph[r[0]:r[-1] + 1, c[0]:c[-1] + 1] = v.astype(np.uint8)
    return out


def compose_f64(photos, rows, faces, inv_ramp, S):
    """The same rule in float64, written from the formulas (weights (1 - t), t on the taps; (1 - a) p + a g)."""
    out = [np.array(p, dtype=np.uint8, copy=True) for p in photos]
    faces = np.asarray(faces, dtype=np.float64)
    inv_ramp = np.asarray(inv_ramp, dtype=np.float64)
    for b, (img, y0, x0, y1, x1) in enumerate(np.asarray(rows).tolist()):
        ph = out[img]
        r, c = _clip_box((y0, x0, y1, x1), ph.shape[0], ph.shape[1])
        if not len(r) or not len(c):
            continue
        ih, iw = y1 - y0, x1 - x0
        fy = (r - y0) * (S - 1.0) / (ih - 1.0) if ih > 1 else np.zeros(len(r))
        fx = (c - x0) * (S - 1.0) / (iw - 1.0) if iw > 1 else np.zeros(len(c))
        yl, xl = np.minimum(np.floor(fy).astype(np.int64), S - 1), np.minimum(np.floor(fx).astype(np.int64), S - 1)
        yh, xh = np.minimum(yl + 1, S - 1), np.minimum(xl + 1, S - 1)
        ty, tx = (fy - yl)[:, None, None], (fx - xl)[None, :, None]
        f = faces[b, :, :, :3]
        g = ((1 - ty) * ((1 - tx) * f[yl][:, xl] + tx * f[yl][:, xh]) + ty * ((1 - tx) * f[yh][:, xl] + tx * f[yh][:, xh]))
        g = np.clip(g, 0.0, 255.0)
        wy = np.minimum(1.0, (np.minimum(r - y0, y1 - 1 - r) + 0.5) * inv_ramp[b, 0])
        wx = np.minimum(1.0, (np.minimum(c - x0, x1 - 1 - c) + 0.5) * inv_ramp[b, 1])
        a = (wy[:, None] * wx[None, :])[:, :, None]
        p = ph[r[0]:r[-1] + 1, c[0]:c[-1] + 1].astype(np.float64)
        ph[r[0]:r[-1] + 1, c[0]:c[-1] + 1] = np.rint((1 - a) * p + a * g).astype(np.uint8)
    return out


def box_mask(photos, rows):
    """Per photo a bool [h, w]: the pixels inside at least one of its boxes."""
    masks = [np.zeros(p.shape[:2], dtype=bool) for p in photos]
    for img, y0, x0, y1, x1 in np.asarray(rows).tolist():
        masks[img][max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = True
    return masks


def pack(photos):
    """u8 [h, w, 3] photos back to back with 16-byte aligned starts (inference.pack_u8's layout): (buffer u8, offsets i64, hw i32);
    the padding bytes hold 0xA5 so that a write into them shows."""
    offs, total = [], 0
    for p in photos:
        offs.append(total)
        total += (p.size + 15) & ~15
    buf = np.full(max(total, 16), 0xA5, dtype=np.uint8)
    for p, o in zip(photos, offs):
        buf[o:o + p.size] = p.reshape(-1)
    return buf, np.array(offs, dtype=np.int64), np.array([p.shape[:2] for p in photos], dtype=np.int32)


def unpack(buf, photos):
    """The photos of a packed buffer (shapes of `photos`) as a list of arrays."""
    _b, offs, _hw = pack(photos)
    buf = np.asarray(buf)
    return [buf[o:o + p.size].reshape(p.shape) for o, p in zip(offs, photos)]


# The rows of the kernel parity test at S = 16: every way a box can meet a photo.  Photos 0..2 are 23 x 37, 40 x 40 and 9 x 64 (odd
# widths: photo rows start at any byte); photo 3 has no box.  Rows 2, 6 and 10 overlap each other on photo 1 and are given out of
# spatial order, with rows of other photos between them; the magnifying box (row 4) lies under all three.
KERNEL_PHOTOS = [(23, 37), (40, 40), (9, 64), (7, 5)]
KERNEL_ROWS = [
    (0, 3, 5, 19, 21),        # 0   16 x 16: the identity scale
    (2, 4, 20, 5, 29),        # 1   1 x 9: ih == 1
    (1, 18, 2, 36, 26),       # 2   overlap C
    (0, -6, 24, 8, 36),       # 3   over the top edge
    (1, 0, 4, 40, 35),        # 4   40 x 31: magnify
    (2, 2, 50, 7, 57),        # 5   5 x 7: minify
    (1, 10, 10, 30, 30),      # 6   overlap A
    (2, 0, 40, 9, 41),        # 7   9 x 1: iw == 1
    (0, 18, 0, 30, 9),        # 8   over the bottom edge (and a corner of row 0)
    (1, 50, 50, 70, 80),      # 9   wholly outside
    (1, 5, 20, 25, 38),       # 10  overlap B
    (2, 1, -5, 8, 6),         # 11  over the left edge
    (2, 3, 58, 12, 70),       # 12  over the right and the bottom edge
]
OVERLAPPING = (2, 6, 10)
# Seeds for which compose_f32 and compose_f64 meet the cap (at most 1 grey level anywhere, at most 0.5 % of box pixels) for every
# feather of the tests: checked on the CPU by test_compose_cpu.test_f32_restatement_against_f64
KERNEL_SEED = 7


def kernel_case(seed=KERNEL_SEED, ld=3):
    """(photos, rows int32 [n, 5], faces f32 [n, 16, 16, ld]): random u8 photos (photo 3 grey), faces uniform in [-60, 315] (so some
    values clip at either end); the channels beyond the third hold NaN, which a kernel that read them would carry into the photo."""
    rng = np.random.RandomState(seed)
    photos = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in KERNEL_PHOTOS]
    photos[3] = np.repeat(photos[3][:, :, :1], 3, axis=2)
    rows = np.array(KERNEL_ROWS, dtype=np.int32)
    faces = np.full((len(rows), S_KERNEL, S_KERNEL, ld), np.nan, dtype=np.float32)
    faces[..., :3] = rng.uniform(-60.0, 315.0, size=(len(rows), S_KERNEL, S_KERNEL, 3)).astype(np.float32)
    return photos, rows, faces


def float_crop(photo, box, S):
    """The box cut from the photo as f32 [S, S, 3] for an S x S box wholly inside it (the crop at the identity scale)."""
    y0, x0, y1, x1 = box
    assert (y1 - y0, x1 - x0) == (S, S) and y0 >= 0 and x0 >= 0 and y1 <= photo.shape[0] and x1 <= photo.shape[1]
    return photo[y0:y1, x0:x1].astype(np.float32)
