"""Data of the photo-ingest kernel tests (tests/test_ingest_gpu.py), built and checked without a GPU (tests/test_ingest_cpu.py).

Exact thin-plate-spline warps: when W - 1 and H - 1 are powers of two the basis rows x = -1 + 2 i / (W - 1) and y are exact in f32 and
0.5 * (W - 1) is a power of two.  With all-zero radial rows and an affine part that is an integer shift (constant row
(2 dx / (W - 1), 2 dy / (H - 1))), optionally with a flip in x or in y (coefficient -1), every sampling coordinate is an integer: three
taps have weight 0 and the output is the shifted or flipped image with exact zeros outside.  Pixels are integers 1..255, so a zero in
the expectation is always the padding.

Exact align warps: S = 128, a power-of-two So and m3 = 3; the constant coefficient a multiple of 8 / S (a shift of 4 crop pixels), +-1
on the q_y -> y and q_x -> x entries, integer (y0, x0) and sy, sx in {0.25, 0.5, 1}.  The crop coordinate of output pixel i is then
4 k + (S / So) i (or 128 + 4 k - (S / So) i), a multiple of 4, and the source coordinate an integer.  (A shift that is not a multiple
of 1 / sy crop pixels would break this: the table keeps to multiples of 4.)

Tight photo buffers: pack_tight() puts the photos back to back behind one leading byte, so every photo starts at an odd byte and the
last one ends on the last byte of the buffer.  Through guarded.inp() that byte is followed by the 0xFF guard band; the tight photos
hold values <= 63, so a guard (or leading) byte that enters a tap with a non-zero weight changes a bit-exact result.
"""
import numpy as np

S = 128

# (B, H, W, C, hc, wc): H * W is never a multiple of the 256-thread block (a partial last block), the batches leave tile tails of
# 3, 1, 2, 3, 5 and 4 samples of 8, and the maps are non-square both ways
TPS_EXACT = [(11, 17, 17, 3, 3, 3), (9, 33, 17, 4, 4, 5), (10, 17, 65, 8, 3, 3), (3, 9, 33, 1, 3, 3), (5, 33, 33, 2, 10, 10),
             (4, 65, 33, 5, 4, 4)]
TPS_EXACT_IDS = ['%dx%dx%dx%d' % s[:4] for s in TPS_EXACT]


def tps_exact_case(B, H, W, C, hc, wc):
    """-> img f32 [B, H, W, C] (integers 1..255, every channel its own pattern), w f32 [B, hc * wc + 3, 2], the index-built expectation
    f32 [B, H, W, C] and inside bool [B, H, W].  Sample b: kind b % 4 of (shift, flip-x + shift, flip-y + shift, identity), its own
    shift (dx, dy) in [-3, 3]^2 (never (0, 0) for the three shifted kinds)."""
    for n in (H, W):
        assert (n - 1) & (n - 2) == 0, 'H - 1 and W - 1 must be powers of two'
    rng = np.random.RandomState(1000 * H + 10 * W + C)
    img = rng.randint(1, 256, size=(B, H, W, C)).astype(np.float32)
    m = hc * wc
    w = np.zeros((B, m + 3, 2), np.float32)
    expect = np.zeros_like(img)
    inside = np.zeros((B, H, W), bool)
    shifts = [(dx, dy) for dx in range(-3, 4) for dy in range(-3, 4) if (dx, dy) != (0, 0)]
    order = [rng.permutation(len(shifts)) for _kind in range(3)]          # per kind: no shift twice
    for b in range(B):
        kind = b % 4
        dx, dy = (0, 0) if kind == 3 else shifts[order[kind][b // 4]]
        ax, ay = (-1 if kind == 1 else 1), (-1 if kind == 2 else 1)
        w[b, m] = (2.0 * dx / (W - 1), 2.0 * dy / (H - 1))          # the constant row: (x, y)
        w[b, m + 1, 0] = ax                                          # x' = ax x + ...
        w[b, m + 2, 1] = ay                                          # y' = ay y + ...
        sx = (np.arange(W) if ax == 1 else W - 1 - np.arange(W)) + dx
        sy = (np.arange(H) if ay == 1 else H - 1 - np.arange(H)) + dy
        ok = ((sy >= 0) & (sy < H))[:, None] & ((sx >= 0) & (sx < W))[None, :]
        expect[b] = np.where(ok[..., None], img[b][np.clip(sy, 0, H - 1)][:, np.clip(sx, 0, W - 1)], np.float32(0))
        inside[b] = ok
    return img, w, expect, inside


# ---- exact align warps ---------------------------------------------------------------------------
ALIGN_PHOTOS = [(96, 130), (128, 128), (31, 47)]          # the 31 x 47 photo last: it ends on the last byte of a tight buffer
ALIGN_SO = [8, 16, 32]                                    # So = 8: one partial block of 64 pixels
# (photo, y0, x0, sy, sx, shift_y, shift_x in units of 4 crop pixels, flip_y, flip_x): 11 rows = a tile of 8 and a tail of 3
ALIGN_ROWS = [(0, 0, 0, 1.0, 1.0, 0, 0, 0, 0),
              (0, -9, 5, 0.5, 1.0, 2, -3, 0, 1),
              (0, 7, -8, 1.0, 0.5, -4, 5, 1, 0),
              (1, 0, 0, 1.0, 1.0, 3, -2, 0, 0),
              (1, -5, 9, 1.0, 1.0, -6, 4, 1, 1),
              (1, 9, -9, 0.5, 0.5, 8, 6, 0, 1),
              (2, 0, 0, 0.25, 0.25, 0, 0, 0, 0),
              (2, -3, -4, 0.25, 0.5, 1, -2, 1, 0),
              (2, 2, 6, 0.5, 0.25, -3, 2, 0, 1),
              (0, -2, 3, 1.0, 1.0, 5, 7, 1, 1),
              (2, -9, -9, 0.25, 0.25, 4, 4, 0, 0)]
ALIGN_K = 10                                              # landmarks of the template that carries the same maps as a tps set


def align_photos(rng_seed=7, high=64):
    rng = np.random.RandomState(rng_seed)
    return [rng.randint(1, high, size=(h, w, 3)).astype(np.uint8) for h, w in ALIGN_PHOTOS]


def align_f32_sources(n=len(ALIGN_ROWS)):
    """f32 [n, S, S, 3], not u8-valued: integers + 0.25."""
    return (np.random.RandomState(8).randint(1, 256, size=(n, S, S, 3)) + 0.25).astype(np.float32)


def align_exact_maps(So):
    """-> owner i64 [n], geom f32 [n, 4] (y0, x0, sy, sx), coef f32 [n, 3, 2] (rows 1, q_y, q_x; columns y, x) and the integer source
    coordinates rows [n, So], cols [n, So] of the output grid."""
    assert S % So == 0 and (So & (So - 1)) == 0
    n = len(ALIGN_ROWS)
    owner = np.array([r[0] for r in ALIGN_ROWS], np.int64)
    geom = np.array([r[1:5] for r in ALIGN_ROWS], np.float32)
    coef = np.zeros((n, 3, 2), np.float32)
    rows, cols = np.zeros((n, So), np.int64), np.zeros((n, So), np.int64)
    i = np.arange(So) * (S // So)
    for b, (_img, y0, x0, sy, sx, ky, kx, fy, fx) in enumerate(ALIGN_ROWS):
        # T(q) = c + s q with q = -1 + 2 i / So: (T + 1) / 2 * S = 4 k + (S / So) i, or 4 k + S - (S / So) i when flipped
        coef[b, 0] = (ky * 8.0 / S, kx * 8.0 / S)
        coef[b, 1, 0] = -1.0 if fy else 1.0
        coef[b, 2, 1] = -1.0 if fx else 1.0
        cy = 4 * ky + (S - i if fy else i)
        cx = 4 * kx + (S - i if fx else i)
        ry, rx = y0 + cy * sy, x0 + cx * sx
        assert np.array_equal(ry, np.rint(ry)) and np.array_equal(rx, np.rint(rx)), 'row %d: a source coordinate is not an integer' % b
        rows[b], cols[b] = ry.astype(np.int64), rx.astype(np.int64)
    return owner, geom, coef, rows, cols


def align_expect(images, owner, rows, cols):
    """The index-built expectation [n, So, So, 3] (the images' dtype as f64) and inside bool [n, So, So]."""
    out, ins = [], []
    for b, i in enumerate(owner):
        im = np.asarray(images[int(i)], np.float64)
        h, w = im.shape[:2]
        ok = ((rows[b] >= 0) & (rows[b] < h))[:, None] & ((cols[b] >= 0) & (cols[b] < w))[None, :]
        out.append(np.where(ok[..., None], im[np.clip(rows[b], 0, h - 1)][:, np.clip(cols[b], 0, w - 1)], 0.0))
        ins.append(ok)
    return np.stack(out), np.stack(ins)


def as_tps_coef(coef3, K=ALIGN_K):
    """The same maps as a tps coefficient set [n, K + 3, 2]: radial rows zero."""
    n = coef3.shape[0]
    return np.concatenate([np.zeros((n, K, 2), np.float32), coef3], axis=1)


# ---- packed u8 photo buffers -------------------------------------------------------------------
def pack_padded(ims):
    """Every photo at a multiple of 16 bytes, gaps zero-filled (as the data loader packs) -> buf u8, offsets i64, hw i32 [n, 2]."""
    offs, total = [], 0
    for im in ims:
        offs.append(total)
        total += (im.size + 15) & ~15
    buf = np.zeros(max(total, 16), np.uint8)
    for im, o in zip(ims, offs):
        buf[o:o + im.size] = im.reshape(-1)
    return buf, np.array(offs, np.int64), np.array([im.shape[:2] for im in ims], np.int32)


def pack_tight(ims, lead=1):
    """Photos back to back with no padding behind `lead` bytes of 0xFF: with lead = 1 and photos of even sizes every start is an odd
    byte, and the last photo ends on the last byte of the buffer -> buf u8, offsets i64, hw i32 [n, 2]."""
    assert all(int(im.max()) <= 63 for im in ims), 'tight photos hold values <= 63 (a 0xFF byte in a tap must show)'
    offs = lead + np.concatenate([[0], np.cumsum([im.size for im in ims])]).astype(np.int64)
    buf = np.full(int(offs[-1]), 0xFF, np.uint8)
    for im, o in zip(ims, offs):
        buf[o:o + im.size] = im.reshape(-1)
    assert offs[-2] + ims[-1].size == buf.size
    return buf, offs[:-1].copy(), np.array([im.shape[:2] for im in ims], np.int32)


PACKERS = {'padded': pack_padded, 'tight': pack_tight}

# photos that imm_resize_crop_u8 down-sizes to FLUSH_RESIZE by exactly 4, 3 and 2: the scale (in - 1) / (out - 1) is an integer, so the
# last output row and column sample the last source row and column with weight 1
FLUSH_RESIZE = (16, 24)
FLUSH_SIZES = [(61, 93), (46, 70), (31, 47)]


# ---- calls the wrappers must refuse ------------------------------------------------------------
def refused_calls(ops, device):
    """[(rule, call)]: one call per rule of ops.tps_warp / tps_warp_pad / resize_crop_u8, each to raise ValueError before any launch.
    Every tensor is a guarded buffer on `device` (tests/guarded.py): nothing may be written, and nothing needs a GPU to be refused."""
    import torch
    import guarded
    f32, B, H, W, C, m3 = torch.float32, 3, 6, 5, 4, 12

    def t(*shape, dtype=f32):
        return guarded.out(shape, dtype, device, fill=0)

    src, basis, w = t(B, H, W, C), t(m3, H * W), t(B, m3, 2)
    dst, c0, rest = t(B, H, W, C), t(B, H, W), t(B, H, W, C - 1)
    tps = ops.tps_warp
    calls = [
        ('tps src dtype', lambda: tps(t(B, H, W, C, dtype=torch.float64), basis, w, dst)),
        ('tps src rank', lambda: tps(t(B, H, W * C), basis, w, dst)),
        ('tps dst dtype', lambda: tps(src, basis, w, t(B, H, W, C, dtype=torch.float16))),
        ('tps dst rank', lambda: tps(src, basis, w, t(B, H, W * C))),
        ('tps dst one sample short', lambda: tps(src, basis, w, t(B - 1, H, W, C))),
        ('tps dst spatial size', lambda: tps(src, basis, w, t(B, W, H, C))),
        ('tps dst too few channels', lambda: tps(src, basis, w, t(B, H, W, C - 1))),
        ('tps dst rows with gaps', lambda: tps(src, basis, w, t(B, H, W + 1, C)[:, :, :W])),
        ('tps dst samples with gaps', lambda: tps(src, basis, w, t(B, H + 1, W, C)[:, :H])),
        ('tps dst channel stride', lambda: tps(src, basis, w, t(B, H, W, 2 * C)[..., ::2])),
        ('tps src rows with gaps', lambda: tps(t(B, H, W + 1, C)[:, :, :W], basis, w, dst)),
        ('tps src channel stride', lambda: tps(t(B, H, W, 2 * C)[..., ::2], basis, w, dst)),
        ('tps dst_c0 rank', lambda: tps(src, basis, w, None, t(B, H, W, 1))),
        ('tps dst_c0 size', lambda: tps(src, basis, w, None, t(B, H, W - 1))),
        ('tps dst_c0 dtype', lambda: tps(src, basis, w, None, t(B, H, W, dtype=torch.float64))),
        ('tps dst_rest too narrow', lambda: tps(src, basis, w, None, c0, t(B, H, W, C - 2))),
        ('tps dst_rest one sample short', lambda: tps(src, basis, w, None, c0, t(B - 1, H, W, C - 1))),
        ('tps dst_rest rows with gaps', lambda: tps(src, basis, w, None, c0, t(B, H, W + 1, C - 1)[:, :, :W])),
        ('tps basis_t transposed', lambda: tps(src, t(H * W, m3), w, dst)),
        ('tps basis_t of another grid', lambda: tps(src, t(m3, H * W - 1), w, dst)),
        ('tps basis_t rows != m3', lambda: tps(src, t(m3 + 1, H * W), w, dst)),
        ('tps basis_t dtype', lambda: tps(src, t(m3, H * W, dtype=torch.float64), w, dst)),
        ('tps basis_t not contiguous', lambda: tps(src, t(m3, 2 * H * W)[:, ::2], w, dst)),
        ('tps w_tps batch', lambda: tps(src, basis, t(B + 1, m3, 2), dst)),
        ('tps w_tps last dim', lambda: tps(src, basis, t(B, m3, 3), dst)),
        ('tps w_tps dtype', lambda: tps(src, basis, t(B, m3, 2, dtype=torch.float64), dst)),
        ('tps w_tps not contiguous', lambda: tps(src, basis, t(B, m3, 4)[..., ::2], dst)),
    ]
    # the padded warp: a 2 x 1 replicate padding, an 8 x 9 grid, the window (1, 2) + 4 x 3
    pad = lambda s, bt, wt, d: ops.tps_warp_pad(s, bt, wt, (1, 2), (8, 9), (1, 2), d)          # noqa: E731
    pbasis, pdst = t(m3, 72), t(B, 4, 3, C)
    calls += [
        ('pad src dtype', lambda: pad(t(B, H, W, C, dtype=torch.float16), pbasis, w, pdst)),
        ('pad dst rank', lambda: pad(src, pbasis, w, t(B, 4, 3 * C))),
        ('pad dst one sample short', lambda: pad(src, pbasis, w, t(B - 1, 4, 3, C))),
        ('pad dst too few channels', lambda: pad(src, pbasis, w, t(B, 4, 3, C - 1))),
        ('pad dst rows with gaps', lambda: pad(src, pbasis, w, t(B, 4, 4, C)[:, :, :3])),
        ('pad basis_t of the unpadded grid', lambda: pad(src, basis, w, pdst)),
        ('pad w_tps batch', lambda: pad(src, pbasis, t(B - 1, m3, 2), pdst)),
    ]
    # resize_crop_u8: 3 photos of 4 x 4 x 3 to 6 x 6, the window (1, 1) + 4 x 4
    u8, offs, hw = t(3 * 48, dtype=torch.uint8), t(3, dtype=torch.int64), t(3, 2, dtype=torch.int32)
    rdst = t(3, 4, 4, 3)
    rs = lambda s, o, h, d, **kw: ops.resize_crop_u8(s, o, h, 3, (6, 6), (1, 1), (4, 4), d, **kw)   # noqa: E731
    calls += [
        ('resize src dtype', lambda: rs(t(3 * 48, dtype=torch.int8), offs, hw, rdst)),
        ('resize offsets dtype', lambda: rs(u8, t(3, dtype=torch.int32), hw, rdst)),
        ('resize offsets length', lambda: rs(u8, t(2, dtype=torch.int64), hw, rdst)),
        ('resize hw dtype', lambda: rs(u8, offs, t(3, 2, dtype=torch.int64), rdst)),
        ('resize hw shape', lambda: rs(u8, offs, t(3, 3, dtype=torch.int32), rdst)),
        ('resize dst dtype', lambda: rs(u8, offs, hw, t(3, 4, 4, 3, dtype=torch.float16))),
        ('resize dst rank', lambda: rs(u8, offs, hw, t(3, 4, 12))),
        ('resize dst one sample short', lambda: rs(u8, offs, hw, t(2, 4, 4, 3))),
        ('resize dst spatial size', lambda: rs(u8, offs, hw, t(3, 4, 3, 3))),
        ('resize dst too few channels', lambda: rs(u8, offs, hw, t(3, 4, 4, 2))),
        ('resize dst rows with gaps', lambda: rs(u8, offs, hw, t(3, 4, 5, 3)[:, :, :4])),
        ('resize dst not dense at ld_dst', lambda: rs(u8, offs, hw, rdst, ld_dst=4)),
        ('resize dst one box row short', lambda: rs(u8, offs, hw, rdst, boxes=t(4, 5, dtype=torch.int32))),
    ]
    return calls
