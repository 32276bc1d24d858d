"""The front of the perceptual VGG (imm_amd/csrc/vgg_first.hip, vgg_head.hip) and the two resampling kernels of
imm_amd/csrc/elementwise.hip (2x2 max pool, align-corners resize) in numpy f64, with a-priori rounding bounds, f32 emulations that can
be made wrong on purpose, and the data of tests/test_vggfront_cpu.py and tests/test_vggfront_gpu.py.  No autograd, no GPU; torch only
rounds to bf16 / f16.

The rule
    pool        y = max of the 2x2 window;  dx = dy at the FIRST maximal position in the order (0,0) (0,1) (1,0) (1,1) (strict >, so
                +0 and -0 tie), +0 elsewhere;  relu_mask: dy counts only where the maximum is > 0
    ac_coord    scale = f32(n_in - 1) / f32(n_out - 1) (0 when n_out == 1);  src = f32(o scale);  lo = floor(src);
                hi = min(lo + 1, n_in - 1);  lerp = src - lo   — all in f32, as the kernel takes them; the lerp itself in f64:
    resize      top = tl + (tr - tl) lx;  bot = bl + (br - bl) lx;  y = top + (bot - top) ly
    resize_bwd  dx[i, j] = sum over (Y, X) of wy wx dy[Y, X],  wy = [y0 == i](1 - ly) + [y1 == i] ly,  wx alike
    gray        g = (p0 + p1 + p2) / 3 / 255 - 114.451 / 255
    conv1_1     a = relu(b + sum_t g[p + t] w[t]),  3x3 SAME, g = 0 outside the image (the NORMALISED gray is padded, not the pixels)
    conv1_1_bwd dgray[p] = sum_t sum_c dz[p - t][c] w[t][c];  dpred[p][ch < 3] = dgray / (3 255) + coef mask e,  e = pred - gt or its
                sign (l1);  no direct term when input_idx < 0;  channels 3 .. lddp - 1 are +0
    head        conv1_1 from 16-bit pairs g = ghi + glo, w = whi + wlo, as whi ghi + whi glo + wlo ghi on the matrix cores, the bias
                the same way against a constant 1;  a11 = RNE16(relu(.));  y12 = RNE16(relu(b12 + conv3x3(a11 as stored, w12)))

Bounds.  u = 2^-24 (half an ulp of f32, relative).  One rounding per f32 operation, a contracted multiply-add has fewer, never more; a
division is taken as good to 1 ulp = 2 u.  Every bound is multiplied by 1 + 2^-10 for the second-order terms a first-order count drops,
and a 16-bit store adds half an ulp of the stored type at |ref| + bound (bn_reference.violations).  All magnitudes are the f64
reference's own.

    resize      top: the difference (1 on |tr - tl|), the product (1 on |tr - tl| lx <= |tr - tl|), the sum (1 on |top|); bot alike;
                y: the errors of top and bot pass with weights 1 - ly and ly (taken as their sum), the difference (1 on |bot - top|),
                the product (1), the sum (1 on |y|):
                    u (2 |tr - tl| + |top| + 2 |br - bl| + |bot| + 2 |bot - top| + |y|)
                plus a contraction allowance: src - lo may be taken as fma(o, scale, -lo), which differs from the restated lerp by the
                rounding of src, at most u src: u (src_x (|tr - tl| + |br - bl|) + src_y |bot - top|)
    resize_bwd  wy: 1 - ly (1) and, where y0 == y1, the sum (1): 2 relative; wx alike; wy wx (1); the product with dy (1): 6 on every
                term, and n - 1 additions (n = the terms of the pixel's stencil) on at most the sum of the absolute terms T:
                    u (6 + n) T,  T = sum |wy wx dy|     plus the allowance  u sum (src_Y wx + wy src_X) |dy|
    gray        two additions (1 each on at most the sum), / 3 (2), / 255 (2): 6 on q = (p0 + p1 + p2) / 765;  the constant is
                114.451f / 255.0f folded in f32 (2 on c);  the subtraction (1 on |g|):   e_g = u (6 q + 2 c + |g|)
    conv1_1     nine multiply-adds from the bias, each 1 on at most A = |b| + sum |g w|:   9 u A + sum_t |w[t]| e_g[p + t]
                With the structured bank (one tap +-2^k, zero bias: every multiply-add exact) that is a handful of f32 ulps.
    conv1_1_bwd exact operands: the 576-term contraction is an integer below 2^24 in any order and through dot2, coef mask e is dyadic;
                what rounds is part / 765 (2 on |dg|) and the one addition (1 on |o|, none where the direct term is 0):
                    u (2 |dg| + [direct != 0] |o|)
    head a11    P = significant bits of the storage type (8 bf16, 11 f16), h = 2^-P the relative half ulp.  x = xhi + xlo + rho_x with
                |xlo| <= h |x| and |rho_x| <= h |xlo| <= h^2 |x|, so  w g - (whi ghi + whi glo + wlo ghi) = wlo glo + rho_w g + w rho_g
                up to third order: 3 h^2 |w g| per tap; the bias against the constant 1: h^2 |b|.  f16: a lo part below 2^-14 is
                subnormal and rounds to 2^-25 absolute instead: + 2^-25 (|w| + |g|) per tap and 2^-25 for the bias (bf16 has f32's
                exponent range: nothing).  The products of 16-bit values are exact in f32; the two chained 32-slot matrix instructions
                add at most 64 roundings on A (1 + 2 h) (the hi/lo cross terms carry A twice more, times h).  The gray word is the VALU
                kernel's f32 value, bit for bit: its e_g passes through |w|.
                    sum_t |w[t]| e_g + 3 h^2 sum |w g| + h^2 |b| + 64 u A (1 + 2 h) [+ 2^-25 (sum (|w| + |g|) + 1)]
    head y12    from the stored a11, taken as an operand: 576 products exact in f32, 18 chained 32-slot matrix instructions, the bias:
                    u (576 T + |y|),  T = sum |w12 a11| + |b12|
                from the images (the bound of a11 carried): every a11 is off by at most e_a + half an ulp of its type, so
                    sum |w12| (e_a + half_ulp(|a11| + e_a)) + u (576 T + |y|)
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_data as E                                                                            # noqa: E402
from bn_reference import F64, STORAGE, STORAGE_IDS, U, exact_in_f32, half_ulp, ratio, store, stored_bits, violations, widen  # noqa: E402,F401
from loss_reference import unpool, window_argmax                                                   # noqa: E402

SLACK = 1.0 + 2.0 ** -10
BF16, F16, F32T = STORAGE
SIXTEEN = [BF16, F16]
SIXTEEN_IDS = ['bf16', 'f16']
PBITS = {BF16: 8, F16: 11}
F32 = np.float32
_cache = {}


def clear_cache():
    _cache.clear()


def cached(key, fn):
    """Built once per process and shared; callers must not modify what they get."""
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def T64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F64))


# ----------------------------------------------------------------------------------------------
# the two comparisons (shared by the GPU tests and by the CPU tests that show they can fail)
# ----------------------------------------------------------------------------------------------
def same(got, v64, dt, what):
    """got holds, bit for bit, what a kernel stores for the exact value v64: v64 itself in f32, its one RNE in a 16-bit type."""
    want = stored_bits(v64, dt)
    E.exact_equal(got, want, what, exact=T64(v64) if want.dtype == torch.int16 else None)


def held(got, ref, bound, dt, what, out=print):
    """No element of got (a tensor of type dt, or f64 values) further from ref than bound (+ half an ulp of a 16-bit dt); nothing is
    left out.  Prints and returns the largest err / tolerance."""
    g = widen(got) if isinstance(got, torch.Tensor) else np.asarray(got, F64)
    g = g.reshape(np.shape(ref))
    bad = violations(g, ref, bound, dt)
    r = ratio(g, ref, bound, dt)
    out('%-58s err/bound %.3f' % (what, r))
    if bad.any():
        i = tuple(int(k) for k in np.argwhere(bad)[0])
        raise AssertionError('%s: %d/%d elements outside their bound (%d not finite), largest err/bound %.3g, first at %s: got %r ref %r bound %.3g' % (
            what, int(bad.sum()), bad.size, int((~np.isfinite(g)).sum()), r, i, float(g[i]), float(np.asarray(ref)[i]),
            float(np.broadcast_to(bound, np.shape(ref))[i])))
    return r


def rounded(v, dt, how='rne'):
    """The f32 values v as a store of type dt leaves them, as f64: 'rne', or the wrong 'trunc' / 'away' (ties away from zero)."""
    v = np.asarray(v, F32)
    if dt == F32T:
        return v.astype(F64)
    rne, trunc, away, _i, _t = E.roundings(torch.from_numpy(v.astype(F64)), dt)
    bits = {'rne': rne, 'trunc': trunc, 'away': away}[how]
    return bits.view(dt).to(torch.float64).numpy()


# ----------------------------------------------------------------------------------------------
# 1. 2x2 max pool
# ----------------------------------------------------------------------------------------------
POOL_SHAPES = [(2, 4, 6, 8), (1, 2, 2, 24)]                                                       # B, h, w, c
POOL_VALUES = [-3.0, -2.0, -1.0, -0.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0]                              # exact in every storage type
_NZ, _PZ = -0.0, 0.0
POOL_WINDOWS = (
    [('unique%d' % q, [3.0 if k == q else v for k, v in enumerate((1.0, -1.0, 0.5, 2.0))]) for q in range(4)] +
    [('tie%d%d' % (i, j), [1.5 if k in (i, j) else v for k, v in enumerate((0.5, -1.0, _PZ, 1.0))])
     for i in range(4) for j in range(i + 1, 4)] +
    [('tie4', [2.0, 2.0, 2.0, 2.0]), ('tie3', [-1.0, 0.5, 0.5, 0.5]),
     ('negative_tie', [-1.0, -3.0, -2.0, -1.0]), ('negative_unique', [-3.0, -2.0, -1.0, -2.0]),
     ('zero_max', [-1.0, _PZ, -2.0, _PZ]), ('zero_all', [_PZ, _PZ, _PZ, _PZ]),
     ('zeros_neg_first', [_NZ, _PZ, -1.0, _NZ]), ('zeros_pos_first', [_PZ, _NZ, _NZ, -2.0]), ('zeros_neg_only', [-1.0, _NZ, _NZ, -3.0])])


def windows_to_map(wins):
    """[B, h/2, w/2, c, 4] (position q = 2 dy + dx) -> [B, h, w, c]."""
    B, h2, w2, c, _ = wins.shape
    return wins.reshape(B, h2, w2, c, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(B, 2 * h2, 2 * w2, c)


def pool_case(B, h, w, c):
    """x: values of POOL_VALUES, every window of POOL_WINDOWS planted once (in a random window and channel), ties frequent in the
    rest; dy: integers in [-5, 5], one in four 0 (+0)."""
    def build():
        g = np.random.RandomState(B * 1000 + h * 100 + w * 10 + c)
        n = B * (h // 2) * (w // 2) * c
        assert n >= len(POOL_WINDOWS)
        wins = np.asarray(POOL_VALUES)[g.randint(0, len(POOL_VALUES), size=(n, 4))]
        at = g.permutation(n)[:len(POOL_WINDOWS)]
        wins[at] = np.asarray([v for _n, v in POOL_WINDOWS])
        wins = wins.reshape(B, h // 2, w // 2, c, 4)
        dy = g.randint(-5, 6, size=(B, h // 2, w // 2, c)).astype(F64)
        dy = np.where(g.random_sample(dy.shape) < 0.25, 0.0, dy)
        return SimpleNamespace(x=windows_to_map(wins), dy=dy, planted=at, shape=(B, h, w, c))
    return cached(('pool', B, h, w, c), build)


def pool_fwd(x):
    _am, w = window_argmax(x)
    return w.max(3)


def pool_bwd(dy, x, relu_mask, last=False):
    """last=True is the WRONG rule (the gradient at the last maximal position)."""
    if relu_mask:
        dy = np.where(pool_fwd(x) > 0, dy, 0.0)
    if not last:
        return unpool(dy, x)
    return unpool(dy[:, ::-1, ::-1], x[:, ::-1, ::-1])[:, ::-1, ::-1]                # the flipped map reverses the order in every window


# ----------------------------------------------------------------------------------------------
# 2. resize, align corners
# ----------------------------------------------------------------------------------------------
def ac_coord(n_in, n_out):
    """-> lo, hi (int), lerp, src (f64 copies of the f32 values)."""
    scale = F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
    src = np.arange(n_out).astype(F32) * scale
    assert src.dtype == F32
    lo = np.floor(src).astype(np.int64)
    hi = np.minimum(lo + 1, n_in - 1)
    lerp = src - lo.astype(F32)
    assert lerp.dtype == F32
    return lo, hi, lerp.astype(F64), src.astype(F64)


def half_pixel_coord(n_in, n_out):
    """The WRONG rule: src = (o + 1/2) n_in / n_out - 1/2, clamped at 0."""
    src = np.maximum((np.arange(n_out).astype(F32) + F32(0.5)) * (F32(n_in) / F32(n_out)) - F32(0.5), F32(0))
    lo = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    hi = np.minimum(lo + 1, n_in - 1)
    return lo, hi, (src - lo.astype(F32)).astype(F64), src.astype(F64)


def _corners(x, ho, wo, coord):
    y0, y1, ly, sy = coord(x.shape[1], ho)
    x0, x1, lx, sx = coord(x.shape[2], wo)
    tl, tr, bl, br = x[:, y0][:, :, x0], x[:, y0][:, :, x1], x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    return tl, tr, bl, br, lx[None, None, :, None], ly[None, :, None, None], sx[None, None, :, None], sy[None, :, None, None]


def resize_fwd(x, ho, wo, coord=ac_coord):
    """x [B, hi, wi, c] f64 -> SimpleNamespace(y, bound, and the partial results)."""
    tl, tr, bl, br, lx, ly, sx, sy = _corners(np.asarray(x, F64), ho, wo, coord)
    r = SimpleNamespace(dt_=tr - tl, db_=br - bl)
    r.pt, r.pb = r.dt_ * lx, r.db_ * lx
    r.top, r.bot = tl + r.pt, bl + r.pb
    r.dv = r.bot - r.top
    r.pv = r.dv * ly
    r.y = r.top + r.pv
    a = np.abs
    r.bound = SLACK * U * (2 * a(r.dt_) + a(r.top) + 2 * a(r.db_) + a(r.bot) + 2 * a(r.dv) + a(r.y) +
                           sx * (a(r.dt_) + a(r.db_)) + sy * a(r.dv))
    return r


def resize_matrix(n_in, n_out, coord=ac_coord):
    """W [n_out, n_in] with y = W x along the axis, and C: u src at the entries of every stencil (the contraction allowance)."""
    lo, hi, lerp, src = coord(n_in, n_out)
    W, C = np.zeros((n_out, n_in)), np.zeros((n_out, n_in))
    o = np.arange(n_out)
    np.add.at(W, (o, lo), 1.0 - lerp)
    np.add.at(W, (o, hi), lerp)
    C[o, lo] = C[o, hi] = U * src
    return W, C


def resize_bwd(dy, hi, wi, coord=ac_coord):
    """dy [B, ho, wo, c] f64 -> SimpleNamespace(dx, bound, terms: the sum of the absolute terms of every element)."""
    dy = np.asarray(dy, F64)
    Wy, Cy = resize_matrix(hi, dy.shape[1], coord)
    Wx, Cx = resize_matrix(wi, dy.shape[2], coord)
    ein = lambda a, d, b: np.einsum('Yi,bYXc,Xj->bijc', a, d, b)                                   # noqa: E731
    r = SimpleNamespace(dx=ein(Wy, dy, Wx), terms=ein(Wy, np.abs(dy), Wx), wy=Wy, wx=Wx)
    n = np.outer((Wy != 0).sum(0), (Wx != 0).sum(0))[None, :, :, None]
    r.bound = SLACK * (U * (6 + n) * r.terms + ein(Cy, np.abs(dy), Wx) + ein(Wy, np.abs(dy), Cx))
    return r


def resize_fwd_f32(x, ho, wo, coord=ac_coord, mid=None):
    """The kernel's arithmetic in numpy f32, without contraction.  mid: a 16-bit type the horizontal lerps are WRONGLY rounded to."""
    tl, tr, bl, br, lx, ly, _sx, _sy = _corners(np.asarray(x, F32), ho, wo, coord)
    lx, ly = lx.astype(F32), ly.astype(F32)
    top, bot = tl + (tr - tl) * lx, bl + (br - bl) * lx
    if mid is not None:
        top, bot = rounded(top, mid).astype(F32), rounded(bot, mid).astype(F32)
    y = top + (bot - top) * ly
    assert y.dtype == F32
    return y


# exact cases: hi, wi, ho, wo.  Every ratio (n_in - 1) / (n_out - 1) is dyadic, so every lerp is a multiple of 1/4 and every weight of
# 1/16: 5->9 (1/2), 9->5 (2), 3->9 (1/4), 9->3 (4), 17->5 (4), 4->4 (1), and the degenerate 1->4, 4->1, 1->1 along one axis
RESIZE_BOTH_FRACTIONAL = [(5, 3, 9, 9), (3, 5, 9, 9)]                                             # weights k/16 with k odd
RESIZE_EXACT = RESIZE_BOTH_FRACTIONAL + [(5, 9, 9, 5), (9, 5, 5, 9), (3, 9, 9, 3), (9, 3, 3, 9), (17, 4, 5, 4), (4, 17, 4, 5),
                (1, 5, 4, 9), (5, 1, 9, 4), (4, 9, 1, 5), (9, 4, 5, 1), (1, 3, 1, 9), (3, 1, 9, 1)]
RESIZE_EXACT_B, RESIZE_EXACT_C, RESIZE_EXACT_LDX, RESIZE_EXACT_LDY = 2, 8, 16, 24
RESIZE_AMP = {BF16: 250, F16: 2000, F32T: 2000}                                                   # the 16-bit store must round


def resize_exact_case(hi, wi, ho, wo, dt):
    def build():
        g = np.random.RandomState(hi * 1000 + wi * 100 + ho * 10 + wo + RESIZE_AMP[dt])
        amp = RESIZE_AMP[dt]
        e = SimpleNamespace(x=g.randint(-amp, amp + 1, size=(RESIZE_EXACT_B, hi, wi, RESIZE_EXACT_C)).astype(F64),
                            dy=g.randint(-amp, amp + 1, size=(RESIZE_EXACT_B, ho, wo, RESIZE_EXACT_C)).astype(F64))
        e.fwd, e.bwd = resize_fwd(e.x, ho, wo), resize_bwd(e.dy, hi, wi)
        return e
    return cached(('resize_exact', hi, wi, ho, wo, dt), build)


# bounded cases: B, hi, wi, ho, wo, c, ldx, ldy.  32 -> 16 is the engine's own ratio (31/15); 12 x 20 -> 7 x 16: unequal ratios
RESIZE_BOUNDED = [(2, 32, 32, 16, 16, 8, 8, 16), (2, 32, 32, 16, 16, 16, 24, 16), (2, 7, 7, 16, 16, 8, 16, 8), (2, 16, 16, 7, 7, 16, 16, 24),
                  (2, 12, 20, 7, 16, 8, 16, 16)]


def resize_bounded_case(B, hi, wi, ho, wo, c, dt):
    def build():
        g = np.random.RandomState(hi * 131 + wi * 17 + ho * 7 + wo + c)
        e = SimpleNamespace(x_t=store(g.standard_normal((B, hi, wi, c)), dt), dy_t=store(g.standard_normal((B, ho, wo, c)), dt))
        e.x, e.dy = widen(e.x_t), widen(e.dy_t)
        e.fwd, e.bwd = resize_fwd(e.x, ho, wo), resize_bwd(e.dy, hi, wi)
        return e
    return cached(('resize_bounded', B, hi, wi, ho, wo, c, dt), build)


# ----------------------------------------------------------------------------------------------
# 3. gray + conv1_1 forward
# ----------------------------------------------------------------------------------------------
C_GRAY = 114.451 / 255.0


def gray(img):
    """img [N, s, s, 3] f64 -> (g, e_g) [N, s, s]."""
    img = np.asarray(img, F64)
    tot = img[..., 0] + img[..., 1] + img[..., 2]
    g = tot / 3.0 / 255.0 - C_GRAY
    return g, U * (6 * np.abs(tot) / 765.0 + 2 * C_GRAY + np.abs(g))


def conv3x3(g, w9, pad=0.0):
    """g [N, s, s], w9 [9, co] (tap t = 3 ky + kx) -> [N, s, s, co]: SAME, `pad` outside the image."""
    N, s, _ = g.shape
    gp = np.full((N, s + 2, s + 2), pad, F64)
    gp[:, 1:-1, 1:-1] = g
    out = np.zeros((N, s, s, w9.shape[1]))
    for t in range(9):
        out += gp[:, t // 3:t // 3 + s, t % 3:t % 3 + s, None] * w9[t]
    return out


def conv1_1(img, w9, b, pad_pixels=False):
    """-> SimpleNamespace(a = relu(conv + b), bound, terms A).  pad_pixels=True is the WRONG padding: zero PIXELS, gray -c, outside."""
    w9, b = np.asarray(w9, F64), np.asarray(b, F64)
    g, e_g = gray(img)
    r = SimpleNamespace(g=g, e_g=e_g)
    r.z = conv3x3(g, w9, -C_GRAY if pad_pixels else 0.0) + b
    r.a = np.maximum(r.z, 0.0)
    r.terms = conv3x3(np.abs(g), np.abs(w9)) + np.abs(b)
    r.bound = SLACK * (9 * U * r.terms + conv3x3(e_g, np.abs(w9)))
    return r


def gray_f32(img):
    img = np.asarray(img, F32)
    g = (img[..., 0] + img[..., 1] + img[..., 2]) / F32(3) / F32(255) - F32(114.451) / F32(255)
    assert g.dtype == F32
    return g


def conv1_1_f32(img, w9, b, pad_pixels=False):
    """The VALU kernel's arithmetic in numpy f32 (multiply, then add: two roundings where the kernel's fma has one)."""
    g = gray_f32(img)
    N, s, _ = g.shape
    gp = np.full((N, s + 2, s + 2), -(F32(114.451) / F32(255)) if pad_pixels else F32(0), F32)
    gp[:, 1:-1, 1:-1] = g
    w9 = np.asarray(w9, F32)
    acc = np.broadcast_to(np.asarray(b, F32), (N, s, s, w9.shape[1])).copy()
    for t in range(9):
        acc = acc + gp[:, t // 3:t // 3 + s, t % 3:t % 3 + s, None] * w9[t]
    assert acc.dtype == F32
    return np.maximum(acc, F32(0))


FWD_SIDES, FWD_BATCHES, FWD_LDP = [16, 17, 40], [1, 2], [3, 5, 8]       # one tile; one tile + a one-pixel row and column of tiles; 2.5 tiles
FWD_CASES = [(s, B, ldp) for s in FWD_SIDES for B in FWD_BATCHES for ldp in FWD_LDP]


def images(B, s, ldp, seed=0):
    """gt f32 [B, s, s, 3] and pred f32 [B, s, s, ldp] in [0, 255), the columns [3, ldp) of pred NaN; and both as one f64 batch."""
    def build():
        g = np.random.RandomState(B * 100 + s + ldp + 7 * seed)
        gt = torch.from_numpy((g.random_sample((B, s, s, 3)) * 255).astype(F32))
        pred = torch.full((B, s, s, ldp), float('nan'))
        pred[..., :3] = torch.from_numpy((g.random_sample((B, s, s, 3)) * 255).astype(F32))
        # a few saturated and black pixels: the ends of the gray range, and a sum that is exact
        gt[0, 0, 0], gt[0, -1, -1], pred[-1, 0, -1, :3], pred[-1, -1, 0, :3] = 255.0, 0.0, 255.0, 0.0
        return SimpleNamespace(gt=gt, pred=pred, both=np.concatenate([widen(gt), widen(pred[..., :3])], 0))
    return cached(('images', B, s, ldp, seed), build)


def bank(kind):
    """w9 [9, 64], b [64] as f32 arrays.  'random': 0.4 randn, 0.1 randn.  'structured': channel ch holds the one tap ch % 9 of value
    +-2^k (k = -2 .. 1, the sign alternating with ch // 9) and no bias; channels 60 .. 63 hold no tap and the biases 0.75, -0.5,
    0.3, 1e-3."""
    def build():
        if kind == 'random':
            g = np.random.RandomState(311)
            return (0.4 * g.standard_normal((9, 64))).astype(F32), (0.1 * g.standard_normal(64)).astype(F32)
        w, b = np.zeros((9, 64), F32), np.zeros(64, F32)
        for ch in range(60):
            w[ch % 9, ch] = (-1.0) ** (ch // 9) * 2.0 ** ((ch // 3) % 4 - 2)
        b[60:] = [0.75, -0.5, 0.3, 1e-3]
        return w, b
    return cached(('bank', kind), build)


# ----------------------------------------------------------------------------------------------
# 4. conv1_1 backward
# ----------------------------------------------------------------------------------------------
BWD_LD = [(3, 8), (4, 16), (16, 64)]                                                              # ldp, lddp
BWD_CASES = [(s, B, ld) for s in FWD_SIDES for B in FWD_BATCHES for ld in BWD_LD]
BWD_COEF = [7.0, 0.375, -5.0]                                                                     # the direct term reads entry 1
BWD_PARAMS = [(m, idx, l1) for m in (True, False) for idx in (1, -1) for l1 in (False, True)]


def bwd_case(B, s, ldp):
    """dz integers in [-4, 4] (70 % non-zero), w integers in [-3, 3], gt and pred integer pixels in [0, 255] with pred == gt on one
    pixel in four, mask in {0, 1/4, .., 1}; columns [3, ldp) of pred NaN."""
    def build():
        g = np.random.RandomState(B * 100 + s + ldp + 5)
        e = SimpleNamespace()
        dz = g.randint(-4, 5, size=(B, s, s, 64)).astype(F64)
        e.dz = np.where(g.random_sample(dz.shape) < 0.7, dz, 0.0)
        e.w = g.randint(-3, 4, size=(9, 64)).astype(F64)
        e.gt = g.randint(0, 256, size=(B, s, s, 3)).astype(F64)
        e.pred = np.where(g.random_sample((B, s, s, 1)) < 0.25, e.gt, g.randint(0, 256, size=(B, s, s, 3)).astype(F64))
        e.mask = g.randint(0, 5, size=(B, s, s)).astype(F64) / 4
        return e
    return cached(('bwd', B, s, ldp), build)


def conv1_1_bwd(dz, w9, gt, pred, mask, c0, l1):
    """-> SimpleNamespace(part (the integer contraction), dg, direct, o [B, s, s, 3], bound)."""
    B, s = dz.shape[:2]
    part = np.zeros((B, s, s))
    for t in range(9):
        G = dz @ w9[t]                                                       # [B, s, s]: sum over the 64 channels
        oy, ox = t // 3 - 1, t % 3 - 1                                       # dgray[p] += G[p - (oy, ox)]
        ys, xs = slice(max(oy, 0), s + min(oy, 0)), slice(max(ox, 0), s + min(ox, 0))
        yd, xd = slice(max(-oy, 0), s + min(-oy, 0)), slice(max(-ox, 0), s + min(-ox, 0))
        part[:, ys, xs] += G[:, yd, xd]
    r = SimpleNamespace(part=part, dg=part / 765.0)
    d = pred - gt
    if l1:
        d = np.sign(d)
    cm = c0 * (np.ones((B, s, s)) if mask is None else mask)
    r.direct = cm[..., None] * d + 0.0
    r.o = r.dg[..., None] + r.direct
    r.bound = SLACK * U * (2 * np.abs(r.dg)[..., None] + np.where(r.direct != 0, np.abs(r.o), 0.0))
    return r


def conv1_1_bwd_f32(dz, w9, gt, pred, mask, c0, l1):
    """The last two operations in numpy f32 (the contraction is exact: taken from the reference)."""
    r = conv1_1_bwd(dz, w9, gt, pred, mask, c0, l1)
    assert exact_in_f32(r.part) and exact_in_f32(r.direct)
    dg = r.part.astype(F32) / (F32(3) * F32(255))
    return dg[..., None] + r.direct.astype(F32)


# ----------------------------------------------------------------------------------------------
# 5. the head in one launch
# ----------------------------------------------------------------------------------------------
def split16(v, dt):
    """f32 values -> (hi, lo) as f32 arrays: hi = RNE16(v), lo = RNE16(v - hi)."""
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=F32))
    hi = t.to(dt).float()
    lo = (t - hi).to(dt).float()
    return hi.numpy(), lo.numpy()


def head_a11(img, w9, b, dt):
    """conv1_1's activation as the head computes it: the reference of conv1_1() with the bound of the hi + lo split."""
    r = conv1_1(img, w9, b)
    h = 2.0 ** -PBITS[dt]
    w9, b = np.abs(np.asarray(w9, F64)), np.abs(np.asarray(b, F64))
    wg = conv3x3(np.abs(r.g), w9)
    bound = conv3x3(r.e_g, w9) + 3 * h * h * wg + h * h * b + 64 * U * r.terms * (1 + 2 * h)
    if dt == F16:
        bound = bound + 2.0 ** -25 * (w9.sum(0) + conv3x3(np.abs(r.g), np.ones((9, 1))) + 1.0)
    r.bound = SLACK * bound
    return r


def head_a11_f32(img, w9, b, dt, drop=None):
    """The split in numpy f32: the products of 16-bit values are exact in f32, summed tap by tap (hi hi, hi lo, lo hi), then the bias
    pair.  drop='hi_lo' leaves whi glo out (WRONG)."""
    g = gray_f32(img)
    N, s, _ = g.shape
    ghi, glo = split16(g, dt)
    whi, wlo = split16(np.asarray(w9, F32), dt)
    bhi, blo = split16(np.asarray(b, F32), dt)
    pad = lambda a: np.pad(a, ((0, 0), (1, 1), (1, 1)))                                            # noqa: E731
    ghi, glo = pad(ghi), pad(glo)
    acc = np.zeros((N, s, s, 64), F32)
    for t in range(9):
        sl = (slice(None), slice(t // 3, t // 3 + s), slice(t % 3, t % 3 + s), None)
        acc = acc + ghi[sl] * whi[t]
        if drop != 'hi_lo':
            acc = acc + glo[sl] * whi[t]
    acc = acc + bhi
    for t in range(9):
        sl = (slice(None), slice(t // 3, t // 3 + s), slice(t % 3, t % 3 + s), None)
        acc = acc + ghi[sl] * wlo[t]
    acc = acc + blo
    assert acc.dtype == F32
    return np.maximum(acc, F32(0))


HEAD_DEAD = [3, 17, 18, 40, 63]                                             # channels of conv1_1 that the ReLU kills: b11 = -6
HEAD_W12_DENSITY = 1.0 / 16


def head_exact_filters():
    """w11 [9, 64] f32: randn scaled to sum |w| = 1.8 v per channel, v in [0.5, 1]; b11 = 6, and -6 on HEAD_DEAD.  |g| < 0.56, so
    |conv| < 1.01 and every live a11 lies in (4.99, 7.01), every dead one is 0.  w12 [3, 3, 64, 64]: integers in [-3, 3], one in 16
    non-zero (so that the outputs lie where a 16-bit store has ties: 16 .. 128); b12: half-integers in [8, 40]."""
    def build():
        g = np.random.RandomState(977)
        w = g.standard_normal((9, 64))
        w11 = (w / np.abs(w).sum(0) * 1.8 * g.uniform(0.5, 1.0, size=64)).astype(F32)
        assert float(np.abs(w11.astype(F64)).sum(0).max()) <= 1.8
        b11 = np.full(64, 6.0, F32)
        b11[HEAD_DEAD] = -6.0
        w12 = g.randint(-3, 4, size=(3, 3, 64, 64)).astype(F64)
        w12 = np.where(g.random_sample(w12.shape) < HEAD_W12_DENSITY, w12, 0.0)
        b12 = g.randint(16, 81, size=64).astype(F64) / 2
        return SimpleNamespace(w11=w11, b11=b11, w12=w12, b12=b12)
    return cached('head_exact', build)


def head_real_filters(dt):
    """Generic filters: w11 0.4 randn, b11 0.1 randn (f32); w12 0.05 randn as the 16-bit type holds it, b12 0.1 randn (f32)."""
    def build():
        g = np.random.RandomState(978)
        w11, b11 = (0.4 * g.standard_normal((9, 64))).astype(F32), (0.1 * g.standard_normal(64)).astype(F32)
        w12 = widen(store(0.05 * g.standard_normal((3, 3, 64, 64)), dt))
        return SimpleNamespace(w11=w11, b11=b11, w12=w12, b12=(0.1 * g.standard_normal(64)).astype(F32).astype(F64))
    return cached(('head_real', dt), build)


def conv1_2(a11, w12, b12, f32=False):
    """relu(conv3x3 SAME (a11 [N, s, s, 64], zero outside the image) + b12), with the sum of the absolute terms; f64, or f32 for the
    one large case, whose data make f32 exact."""
    from oracle import imm_oracle as O
    tt = torch.float32 if f32 else torch.float64
    a, w, b = (torch.from_numpy(np.ascontiguousarray(v)).to(tt) for v in (a11, w12, b12))
    z = O.conv2d_same(a, w, b)
    r = SimpleNamespace(z=z.double().numpy(), y=z.clamp(min=0).double().numpy())
    if not f32:
        r.terms = O.conv2d_same(a.abs(), w.abs(), b.abs()).numpy()
    return r


def y12_bound_from_stored(r):
    return SLACK * U * (576 * r.terms + np.abs(r.y))


def y12_bound_from_images(ra, r, w12, dt):
    """ra: head_a11(); r: conv1_2(ra.a, ...)."""
    from oracle import imm_oracle as O
    e_a = ra.bound + half_ulp(np.abs(ra.a) + ra.bound, dt)
    carried = O.conv2d_same(T64(e_a), T64(np.abs(w12)), None).numpy()
    return SLACK * carried + y12_bound_from_stored(r)


def head_big_batch(cus, s=128, walks=5):
    """The smallest batch at which each of min(patches, cus) persistent workgroups walks at least `walks` patches of 8 x 16 pixels."""
    per_img = (s // 16) * (s // 8)
    return max(1, -(-walks * cus // (2 * per_img)))
