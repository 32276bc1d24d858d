"""Exact-arithmetic data for the kernel tests: small signed integers in, one answer out, compared bit for bit.

Every operand is a small integer (a bias is a half-integer), so every product is exact in f32 and every partial sum, in any order,
is a multiple of 1/2 below 2^24: the f32 accumulator of a convolution is the mathematically exact value whatever the tiling, the
split or the matrix instruction.  What a kernel stores is then determined to the bit: RNE16(exact) for a 16-bit output, the exact
value for an f32 output, a filter gradient or a batch-norm partial sum.  The f64 CPU convolution of such data is exact as well,
so the reference restates nothing.

make()          seeded integer operands and the f64 references (forward, data gradient, filter gradient), with the sum |x||w|
                bounds that prove the exactness premise for the case.
rne16()         the expected stored bits of an exact f64 value (f64 -> f32 is exact here, and asserted; f32 -> 16 bit is RNE).
exact_equal()   bitwise comparison that names the defect: count, first index, and whether `got` is the truncated or the
                ties-away rounding of the exact value.
rounding_mix()  the fractions of a reference that are not representable / exact ties / inexact non-ties in a 16-bit type.

The case tables of tests/test_exact_gpu.py live here too (FWD_KEY, FWD_HIGH, DGRAD, WGRAD, ...), with the amplitudes chosen per case and type, so that
tests/test_exact_cpu.py validates them on the reference alone.  Nothing here needs a GPU at import.
"""
import os
import sys
from types import SimpleNamespace

import torch

from oracle import imm_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

F64 = torch.float64
LIMIT = float(2 ** 24)
_INT = {2: torch.int16, 4: torch.int32, 8: torch.int64}


def ints(shape, amp, seed, density=1.0, lo=None):
    """Seeded integers in [lo, amp] (lo = -amp by default) as f64; density < 1 zeroes a random share of them."""
    g = torch.Generator().manual_seed(seed)
    lo = -amp if lo is None else lo
    v = torch.randint(lo, amp + 1, tuple(shape), generator=g).to(F64)
    if density < 1.0:
        v = v * (torch.rand(tuple(shape), generator=g) < density)
    return v


def half_ints(n, amp, seed):
    """Bias values k/2 with k in [-2 amp, 2 amp]: channels 1, 5, 9, ... get an odd k, so their outputs are integers plus one half
    (not representable in a 16-bit type from 2^7 up in bf16 and from 2^10 up in f16); the other channels get whole numbers."""
    k = 2 * ints((n,), amp, seed)
    k[1::4] += 1
    return k / 2


def representable(t, dt):
    return bool((t.to(dt).to(F64) == t).all())


def make(shape, dt, amps, density=1.0, seed=0, bias=True, want=('fwd',), kw=None, bounds=False, spike=None):
    """shape = (B, H, W, ci, co, k, stride): a k x k (k x kw) SAME convolution.  amps = (ax, aw): activations (x, and dy of the
    gradients) in [-ax, ax], filter taps in [-aw, aw]; `density` thins x and dy.  Returns f64 tensors:
        x, w, bias (None without), dy (when a gradient is wanted)
        y   conv(x, w) + bias                       ('fwd')
        dx  the data gradient of dy                   ('dgrad')
        dw  the filter gradient of (x, dy)            ('wgrad')
    and with bounds=True y_bound = conv(|x|, |w|) + |bias|, dx_bound, dw_bound: the sum of the absolute terms of every output.
    spike = (A, n): the last input channel (a K-tail channel) carries nothing but n pixels of value A, and only the centre tap of the
    filter reads it (+1 into even output channels, -1 into odd ones): every output channel gets n values near +-A (set_spikes)."""
    B, H, W, ci, co, k, stride = shape
    kw = k if kw is None else kw
    ax, aw = amps
    e = SimpleNamespace(shape=shape, dt=dt, amps=amps, density=density)
    e.x = ints((B, H, W, ci), ax, seed * 10 + 1, density)
    e.w = ints((k, kw, ci, co), aw, seed * 10 + 2)
    e.bias = half_ints(co, 2 * aw, seed * 10 + 3) if bias else None
    if spike is not None:
        set_spikes(e.x, e.w, *spike)
    assert representable(e.x, dt) and representable(e.w, dt), 'operands must be exact in %s' % dt
    if 'fwd' in want:
        e.y = O.conv2d_same(e.x, e.w, e.bias, stride)
        if bounds:
            e.y_bound = O.conv2d_same(e.x.abs(), e.w.abs(), None if e.bias is None else e.bias.abs(), stride)
    if 'dgrad' in want or 'wgrad' in want:
        ho, wo = -(-H // stride), -(-W // stride)
        e.dy = ints((B, ho, wo, co), ax, seed * 10 + 4, density)
        assert representable(e.dy, dt)
    if 'dgrad' in want:
        e.dx = _dgrad(e.dy, e.w, (B, H, W, ci), stride)
        if bounds:
            e.dx_bound = _dgrad(e.dy.abs(), e.w.abs(), (B, H, W, ci), stride)
    if 'wgrad' in want:
        e.dw = _wgrad(e.x, e.dy, e.w.shape, stride)
        if bounds:
            e.dw_bound = _wgrad(e.x.abs(), e.dy.abs(), e.w.shape, stride)
    return e


def set_spikes(x, w, amp, n):
    """In place: input channel ci - 1 becomes zero but for n pixels of value amp at odd coordinates (the first near the start of the
    first image, the second near the end of the last), and the filter reads that channel at its centre tap alone.  With SAME padding
    an odd pixel sits under the centre tap of exactly one output at stride 1 and at stride 2 (even maps: no padding at the top), so
    each output channel holds exactly n values amp * (+-1) + (what the other channels give)."""
    B, H, W, ci = x.shape
    assert H % 2 == 0 and W % 2 == 0 and H >= 4 and W >= 4 and 1 <= n <= 2
    x[..., ci - 1] = 0
    w[:, :, ci - 1, :] = 0
    w[w.shape[0] // 2, w.shape[1] // 2, ci - 1, 0::2] = 1
    w[w.shape[0] // 2, w.shape[1] // 2, ci - 1, 1::2] = -1
    for b, py, px in [(0, 1, 3), (B - 1, H - 3, W - 1)][:n]:
        x[b, py, px, ci - 1] = amp


def _dgrad(dy, w, xshape, stride):
    xr = torch.zeros(xshape, dtype=F64, requires_grad=True)
    (g,) = torch.autograd.grad(O.conv2d_same(xr, w, None, stride), xr, dy)
    return g


def _wgrad(x, dy, wshape, stride):
    wr = torch.zeros(tuple(wshape), dtype=F64, requires_grad=True)
    (g,) = torch.autograd.grad(O.conv2d_same(x, wr, None, stride), wr, dy)
    return g


def rne16(ref64, dt):
    """The bits a kernel must store for the exact value ref64: one round-to-nearest-even from f32 to dt, as int16."""
    assert ref64.dtype == F64
    assert bool(torch.isfinite(ref64).all()), 'the REFERENCE is not finite: a bug of the test, not of the kernel'
    f32 = ref64.float()
    assert bool((f32.to(F64) == ref64).all()), 'the reference is not exact in f32: the amplitudes of this case are too high'
    r = f32.to(dt)
    assert bool(torch.isfinite(r.float()).all()), 'the reference saturates %s: the amplitudes of this case are too high' % dt
    return r.contiguous().view(torch.int16)


def _mag_value(mag, dt):
    """The non-negative dt value with magnitude bits `mag` (int32), as f64."""
    return mag.to(torch.int16).view(dt).to(F64)


def roundings(exact64, dt):
    """(rne, truncated, ties-away) bits of exact64 in dt as int16 tensors, and the masks (inexact, tie)."""
    a = exact64.abs()
    rne = a.float().to(dt)
    mag = rne.contiguous().view(torch.int16).to(torch.int32)
    rv = rne.to(F64)
    inexact = rv != a
    lo = torch.where(rv > a, mag - 1, mag)                     # magnitude bits of the neighbour towards zero
    tie = inexact & ((a - _mag_value(lo, dt)) == (_mag_value(lo + 1, dt) - a))
    away = torch.where(tie, lo + 1, mag)
    sign = torch.where(torch.signbit(exact64), 0x8000, 0).to(torch.int32)

    def bits(m):                                               # sign | magnitude, 0..65535 -> the same 16 bits as int16
        return (((m | sign) + 0x8000) % 0x10000 - 0x8000).to(torch.int16)
    return bits(mag), bits(lo), bits(away), inexact, tie


def rounding_mix(exact64, dt):
    """Fractions (not representable, exact ties, inexact non-ties) of exact64 in dt."""
    _r, _t, _a, inexact, tie = roundings(exact64, dt)
    n = float(exact64.numel())
    return float(inexact.sum()) / n, float(tie.sum()) / n, float((inexact & ~tie).sum()) / n


def exact_equal(got, want, what, exact=None):
    """got == want bit for bit.  `want`: int16 bits (rne16) for a 16-bit `got`, else values of an f32 / f64 `got`.  `exact`: the
    unrounded f64 value behind a 16-bit `want`; with it a failure says whether got is its truncation or its ties-away rounding."""
    got = got.detach().cpu().contiguous()
    want = want.detach().cpu().contiguous()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    if want.dtype == torch.int16:
        assert got.element_size() == 2, (what, got.dtype)
        gb, wb = got.view(torch.int16), want
        wv = want.view(got.dtype).float()
    else:
        assert got.dtype in (torch.float32, torch.float64), (what, got.dtype)
        wv = want.to(got.dtype)
        assert bool((wv.to(F64) == want.to(F64)).all()) or not bool(torch.isfinite(want).all()), \
            '%s: the reference is not exact in %s: a bug of the test' % (what, got.dtype)
        gb, wb = got.view(_INT[got.element_size()]), wv.contiguous().view(_INT[got.element_size()])
    ok = torch.isfinite(wv)
    assert bool(ok.all()), '%s: the REFERENCE holds %d non-finite of %d elements: a bug of the test, not of the kernel' % (
        what, int((~ok).sum()), wv.numel())
    bad = gb != wb
    if not bool(bad.any()):
        return
    gf = got.to(F64)
    idx = tuple(int(i) for i in bad.nonzero()[0])
    msg = '%s: %d/%d elements differ (%d NaN, %d inf in got); first at %s got %r want %r' % (
        what, int(bad.sum()), bad.numel(), int(torch.isnan(gf).sum()), int(torch.isinf(gf).sum()), idx, float(gf[idx]), float(wv[idx]))
    if exact is not None and want.dtype == torch.int16:
        ex = exact.detach().cpu().to(F64)
        _r, trunc, away, _i, _t = roundings(ex, got.dtype)
        n_tr, n_aw = int((gb[bad] == trunc[bad]).sum()), int((gb[bad] == away[bad]).sum())
        kind = ('got is the TRUNCATED exact value' if gb[idx] == trunc[idx] else
                'got is the TIES-AWAY rounding of the exact value' if gb[idx] == away[idx] else
                'got is neither the truncated nor the ties-away rounding: a wrong sum or a second rounding')
        msg += ' (exact %r: %s; of the differing elements %d match truncation, %d ties-away)' % (float(ex[idx]), kind, n_tr, n_aw)
    raise AssertionError(msg)


# ----------------------------------------------------------------------------------------------
# case tables of tests/test_exact_gpu.py (validated on the reference alone by tests/test_exact_cpu.py)
# ----------------------------------------------------------------------------------------------
BF16, F16 = torch.bfloat16, torch.float16
DTYPES = [BF16, F16]
DT_IDS = ['bf16', 'f16']


def fwd_shapes():
    import test_kernels_gpu as K      # the shapes are the suite's own: the dispatch thresholds of a 256-CU part fix them
    cases = {c[-1]: c[:-1] for c in K.CONV_CASES}
    for B, H, ci, co, _bn, tag in K.S2F_CASES:
        cases[tag] = (B, H, ci, ci, co, 3, 2, False)
    return cases


# tag -> (family, variant) of imm_conv2d_variant with IMM_CONV_BIAS (| IMM_CONV_RELU); then what the other flag sets select where
# it is not the same kernel.  None: the entry point refuses the combination (an f32 output excludes the mask).
FWD_KEY = {
    'enc3x3': ('igemm', 110802), 'stride2': ('igemm', 110404), 'first7x7': ('igemm', 100802), 'pose1x1': ('igemm', 110801),
    'concat266': ('igemm', 110404), 'ragged_m100': ('igemm64', 210404), 'vgg5': ('igemm64', 210404),
    'halo_64_64': ('halo2', 406464), 'halo_32_32': ('halo2', 403232),
    'halo_32_9_f32': ('halo', 303216), 'halo_s2_co48': ('halo', 313264),
    'hdeep_bn128_one_slice': ('hdeep6', 600000), 'hdeep_persistent_ragged': ('hdeep6', 600001),
    'hdeep_bn64_two_slices': ('hdeep', 520648), 'hdeep_small_patch': ('hdeep', 520644), 'hdeep_map8': ('hdeep', 560644),
    'hdeep_persistent_bn64': ('hdeep', 510648),
    'one_nblk_two_slices': ('s2f', 700064), 'enc_conv5_64to128': ('s2f', 700128),
}
FWD_TAGS = list(FWD_KEY)
# (tag, run) -> the kernel that serves the run when the family of the tag declines the flags
FWD_KEY_OTHER = {
    ('pose1x1', 'mask'): None, ('pose1x1', 'stats_mask'): None, ('halo_32_9_f32', 'mask'): None, ('halo_32_9_f32', 'stats_mask'): None,
    # the stride-2 LDS-halo forward kernels have no mask: the im2col kernels serve it
    ('halo_s2_co48', 'mask'): ('igemm', 110404), ('halo_s2_co48', 'stats_mask'): ('igemm', 110404),
    ('one_nblk_two_slices', 'mask'): ('igemm64', 210404), ('one_nblk_two_slices', 'stats_mask'): ('igemm64', 210404),
    ('enc_conv5_64to128', 'mask'): ('igemm64', 210804), ('enc_conv5_64to128', 'stats_mask'): ('igemm64', 210804),
    # conv_hdeep6 has no partial sums, and persistent tiles none either: conv_hdeep, one workgroup per tile
    ('hdeep_bn128_one_slice', 'stats'): ('hdeep', 501288), ('hdeep_bn128_one_slice', 'stats_mask'): ('hdeep', 501288),
    ('hdeep_persistent_ragged', 'stats'): ('hdeep', 501288), ('hdeep_persistent_ragged', 'stats_mask'): ('hdeep', 501288),
    ('hdeep_persistent_bn64', 'stats'): ('hdeep', 500648), ('hdeep_persistent_bn64', 'stats_mask'): ('hdeep', 500648),
}


def fwd_key(tag, run):
    return FWD_KEY_OTHER.get((tag, run), FWD_KEY[tag])


# High amplitudes (ax, aw) per case and type: large enough that the 16-bit store rounds (>= 20 % not representable, >= 5 % ties,
# >= 5 % inexact non-ties, after the ReLU and after the mask too), small enough that f16 stays below half its maximum.
FWD_HIGH = {
    'enc3x3': ((16, 8), (64, 16)), 'stride2': ((16, 8), (64, 16)), 'first7x7': ((16, 8), (64, 16)), 'pose1x1': ((8, 4), (32, 16)),
    'concat266': ((8, 4), (32, 8)), 'ragged_m100': ((16, 4), (32, 16)), 'vgg5': ((8, 4), (32, 8)),
    'halo_64_64': ((16, 4), (32, 16)), 'halo_32_32': ((16, 8), (64, 16)), 'halo_32_9_f32': ((8, 4), (32, 16)),
    'halo_s2_co48': ((16, 8), (64, 16)), 'hdeep_bn128_one_slice': ((16, 4), (32, 16)), 'hdeep_persistent_ragged': ((16, 4), (48, 8)),
    'hdeep_bn64_two_slices': ((16, 4), (48, 8)), 'hdeep_small_patch': ((16, 4), (48, 8)), 'hdeep_map8': ((8, 4), (32, 8)),
    'hdeep_persistent_bn64': ((16, 4), (48, 8)), 'one_nblk_two_slices': ((16, 4), (32, 16)), 'enc_conv5_64to128': ((16, 4), (32, 16)),
}
# Low runs (batch-norm partial sums): x and w in [-1, 1], x thinned to this density where the launch-wide sum of v^2 of a channel
# would pass 2^24 / 4 otherwise (many pixels x deep K).
FWD_LOW_DENSITY = {'hdeep_bn128_one_slice': 0.12, 'hdeep_persistent_ragged': 0.03, 'hdeep_bn64_two_slices': 0.25,
                   'hdeep_small_patch': 0.5, 'hdeep_map8': 0.25, 'hdeep_persistent_bn64': 0.015, 'enc_conv5_64to128': 0.25}
LOW_AMPS = (1, 1)
# On such data alone every v is a small number that both 16-bit types hold exactly, and sums taken from the ROUNDED value would
# equal the sums of v.  So each low run also carries a few spikes (set_spikes): values v near +-A that the store does round, in every
# output channel: in bf16 the odd integers above 256 (ties) and the half-integers above 128; in f16 only the half-integers above
# 1024, since an odd integer above 2048 would alone take 4 v^2 past 2^24.  One f16 spike uses 4 x 1100^2 = 4.8e6 of the 1.7e7 that
# a channel's sum of squares may reach, so there is one; bf16 has two, in the first and in the last image.
# Each f16 case then rests on ONE rounding value per half-integer channel: tests/test_exact_cpu.py asserts, per case and type, that
# the sums of the rounded outputs differ from the exact ones, which is what holds a later change of seeds, mask or amplitudes.
LOW_SPIKE = ((300, 2), (1100, 1))


def mask_ints(shape, seed):
    """Integer mask_ref of both signs and zeros (70 % positive, so that most rounded outputs survive it)."""
    return ints(shape, 7, seed, lo=-2)


_cache = {}


def cached(key, fn):
    """References are computed once per process and shared (callers must not modify them)."""
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def fwd_data(tag, dt, low, bounds=False):
    B, H, ci_real, _ci_pad, co, k, stride, _f32 = fwd_shapes()[tag]
    amps = LOW_AMPS if low else FWD_HIGH[tag][DTYPES.index(dt)]
    dens = FWD_LOW_DENSITY.get(tag, 1.0) if low else 1.0

    def build():
        e = make((B, H, H, ci_real, co, k, stride), dt, amps, density=dens, seed=(2 if low else 1), bounds=bounds,
                 spike=(LOW_SPIKE[DTYPES.index(dt)] if low else None))
        e.mask = mask_ints(e.y.shape, 99)
        return e
    return cached(('fwd', tag, dt, low, bounds), build)


# conv_first (the 7x7x3 first convolution from the f32 image): integer pixels 0..ax, taps in [-aw, aw]
FIRST_CASES = [(2, 128, 32), (3, 32, 20)]
FIRST_HIGH = ((48, 8), (96, 16))


def first_data(B, S, co, dt, low, bounds=False):
    ax, aw = (1, 1) if low else FIRST_HIGH[DTYPES.index(dt)]      # low: pixels 0 / 1, four in five of them 0

    def build():
        e = SimpleNamespace()
        e.x = ints((B, S, S, 3), ax, 71, density=(0.2 if low else 1.0), lo=0)
        e.w = ints((7, 7, 3, co), aw, 72)
        e.bias = half_ints(co, 2 * aw, 73)
        if low:
            set_spikes(e.x, e.w, *LOW_SPIKE[DTYPES.index(dt)])
        assert representable(e.x, dt) and representable(e.w, dt)
        e.y = O.conv2d_same(e.x, e.w, e.bias, 1)
        if bounds:
            e.y_bound = O.conv2d_same(e.x.abs(), e.w.abs(), e.bias.abs(), 1)
        return e
    return cached(('first', B, S, co, dt, low, bounds), build)


# data gradients: tag -> (B, H, ci (dx channels), ci_pad, co (dy channels), co_pad, k, stride), (family, variant), amplitudes
DGRAD = {
    'k3s1': ((2, 16, 32, 32, 32, 32, 3, 1), ('igemm', 110802), ((16, 4), (32, 16))),
    'k3s2_b': ((2, 32, 64, 64, 128, 128, 3, 2), ('igemm64', 210404), ((16, 4), (32, 16))),
    'hdeep_256to128': ((16, 32, 128, 128, 256, 256, 3, 1), ('hdeep', 520644), ((8, 4), (32, 8))),
}
GROUP = ((8, 16, 32, 64), ('igemm', 110802), ((16, 8), (64, 16)))                      # B, H, ci, co: four parity classes, one launch
S2D = {'dx8_three_slices': ((1, 32, 8, 192), ((16, 4), (32, 16))), 'halo_form_dx12': ((1, 64, 12, 64), ((16, 8), (64, 16)))}
TAP = {'l1': ((4, 32, 256, 256, True), ((8, 4), (32, 8))), 'l2': ((8, 32, 256, 256, False), ((8, 4), (32, 8)))}
TAP_KEY = ('hdeep', 520644)


def dgrad_data(kind, tag, shape, dt, amps, bounds=False):
    """shape = (B, H, ci, co, k, stride) of the FORWARD convolution whose data gradient is taken."""
    B, H, ci, co, k, stride = shape
    return cached((kind, tag, dt, bounds),
                  lambda: make((B, H, H, ci, co, k, stride), dt, amps[DTYPES.index(dt)], seed=3, bias=False, want=('dgrad',), bounds=bounds))


# filter gradients: x and dy in [-8, 8]; tag -> (B, H, ci_real, ci_pad, co, lddy, k, kw, stride, nsplit (0: the kernel's own), variant)
# imm_conv2d_wgrad_variant names the kernel that serves the descriptor at its OWN split count (it has no split argument).  The
# LDS-halo kernel takes a job at that count alone: 'h32_32_transposed' has the descriptor and so the key of 'h32_32' (203232), and
# at 3 splits, which is not that count (the test asserts so), the entry point gives it to the transpose-read kernel.
WGRAD_AMPS = (8, 1)
WGRAD = {
    'k3s1_split1': (2, 16, 32, 32, 32, 32, 3, 3, 1, 1, 100032), 'k3s1_split5': (2, 16, 32, 32, 32, 32, 3, 3, 1, 5, 100032),
    'general_m100': (1, 10, 64, 64, 64, 64, 3, 3, 1, 2, 0),
    'h32_32': (1, 128, 32, 32, 32, 32, 3, 3, 1, 0, 203232), 'h32_32_transposed': (1, 128, 32, 32, 32, 32, 3, 3, 1, 3, 203232),
    'first_7x1': (2, 64, 32, 32, 32, 32, 7, 1, 1, 0, 210332), 'halo_s2_co48': (1, 64, 32, 32, 48, 64, 3, 3, 2, 0, 223264),
}
# the job list of test_conv_wgrad_multi_equals_single_launches: B, H, ci, co, lddy, k, stride, nsplit; and its variants
WGRAD_MULTI = [(2, 16, 256, 256, 256, 3, 1, 2), (2, 16, 256, 256, 256, 3, 1, 3), (4, 32, 128, 128, 128, 3, 1, 4),
               (2, 32, 64, 128, 128, 3, 2, 2), (2, 64, 32, 64, 64, 3, 2, 5), (1, 128, 32, 32, 32, 3, 1, 7),
               (2, 64, 64, 64, 64, 3, 1, 6), (2, 64, 64, 32, 32, 3, 1, 3), (2, 16, 256, 10, 16, 1, 1, 2),
               (5, 64, 128, 64, 64, 3, 1, 9), (1, 10, 64, 64, 64, 3, 1, 2)]
WGRAD_MULTI_KEYS = [206464, 206464, 206464, 100128, 223264, 203232, 206464, 206432, 100016, 206464, 0]


def wgrad_data(key, B, H, ci, co, k, kw, stride, dt, seed, bounds=False):
    return cached(('wgrad', key, dt, bounds),
                  lambda: make((B, H, H, ci, co, k, stride), dt, WGRAD_AMPS, seed=seed, bias=False, want=('wgrad',), kw=kw, bounds=bounds))


# plain sums that feed the same layers: imm_masked_sse / _pool at (B 3, s 32, c 128) under a 64 x 64 mask, imm_colsum at (c 64, npix 1000)
SSE_SHAPE = (3, 32, 128, 64)
COLSUM_SHAPE = (64, 1000)


def sse_data(dt):
    B, s, c, S = SSE_SHAPE
    a, b, mask = ints((B, s, s, c), 3, 301), ints((B, s, s, c), 3, 302), ints((B, S, S), 3, 303, lo=0)
    assert representable(a, dt) and representable(b, dt)
    return a, b, mask


def colsum_data(dt):
    c, npix = COLSUM_SHAPE
    x = ints((npix, c), 8, 31)
    assert representable(x, dt)
    return x
