"""The front of the perceptual VGG and the two resampling kernels on a real MI355X, bit for bit where the arithmetic allows it and
against f64 within counted bounds where it does not (tests/vgg_reference.py: the rule, the bounds, the data), in every storage type
the entry point dispatches on.

1. imm_maxpool2_fwd/_bwd: selections only, so zero tolerance on any data: every tie kind at positive, zero, signed-zero and negative
   maxima; the gradient at the first maximal position, with and without the ReLU mask, one non-zero per window where dy != 0.
2. imm_resize_ac_fwd/_bwd: integer data at every dyadic ratio and the degenerate sizes (1 -> n, n -> 1, 1 -> 1, the identity), non-
   square, ld > c on both sides: RNE16(exact), and the integer adjoint identity; real data at 31/15 and other ratios within the bound.
3. imm_vgg_conv1_1_fwd within its bound at one tile, one tile + 1 pixel, two and a half tiles, ldp 3 / 5 / 8, with random filters
   and with a bank of single power-of-two taps whose bound is a handful of f32 ulps; halves 1 then 2 == halves 3 bit for bit.
4. imm_vgg_conv1_1_bwd, the 16-bit kernel and the f32 one: integer dz and w, integer pred - gt, a dyadic mask and coefficient, so
   that two f32 roundings remain; mask given and NULL, input_idx -1 and 1, l1 0 and 1, (ldp, lddp) (3, 8) (4, 16) (16, 64).
5. imm_vgg_head_fwd: conv1_1 from the hi + lo split within the split's bound; conv1_2, the copy of the conv_halo2 loop, bit for bit
   from the conv1_1 activation the launch itself stored (live channels in [4, 8), dead ones 0), at one patch per workgroup, at a grid
   that is no multiple of 8 with the non-power-of-two decode, and at a batch taken from the CU count so that every workgroup walks
   five patches (the gray ring wraps, the drain follows a steady state); store_from = B and 2B change no bit of y12 and leave the
   images below untouched; real data against f64.

Every kernel output is a guarded.out() buffer, every operand a guarded.inp() that ends on its guard band, columns the kernel does not
own hold NaN and are asserted untouched.  Every bounded comparison prints its largest err/bound (run with -s); DESIGN.md item 84
records them.  tests/test_vggfront_cpu.py shows without a GPU what the data must satisfy and that each comparison can fail.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded                                                              # noqa: E402
from guarded import untouched                                               # noqa: E402
import vgg_reference as V                                                   # noqa: E402
from vgg_reference import T64, held, same, widen                            # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN = float('nan')
F32 = torch.float32
DT = pytest.mark.parametrize('dt', V.STORAGE, ids=V.STORAGE_IDS)
DT16 = pytest.mark.parametrize('dt', V.SIXTEEN, ids=V.SIXTEEN_IDS)
_BITS = {2: torch.int16, 4: torch.int32}


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from imm_amd import ops as _ops
    torch.cuda.set_device(0)
    return _ops


@pytest.fixture(scope='module', autouse=True)
def _release_cases():
    yield
    V.clear_cache()


@pytest.fixture(autouse=True)
def _guards_intact():
    """After every test: no kernel wrote outside a tensor it was handed (tests/guarded.py)."""
    guarded.reset()
    yield
    guarded.check_guards()


def dev(t):
    return guarded.inp(t, DEV, depth=2)


def wide(t, ld):
    """[..., c] -> [..., ld] with NaN in the columns [c, ld), as a guarded operand."""
    if ld != t.shape[-1]:
        o = torch.full(tuple(t.shape[:-1]) + (ld,), NAN, dtype=t.dtype)
        o[..., :t.shape[-1]] = t
        t = o
    return guarded.inp(t, DEV, depth=2)


def put(v64, dt, ld=None):
    """Exact f64 data as a guarded operand of type dt (asserted representable), `ld` wide when given."""
    t = V.store(v64, dt)
    assert torch.equal(t.double(), T64(v64)), 'not representable in %s' % dt
    return wide(t, t.shape[-1] if ld is None else ld)


def gout(shape, dt, fill=None):
    return guarded.out(shape, dt, DEV, fill=fill, what=guarded._caller(1))


def bits(t):
    return t.contiguous().view(_BITS[t.element_size()])


# ==============================================================================================
# 1. 2x2 max pool: bit for bit on any data
# ==============================================================================================
@DT
@pytest.mark.parametrize('B,h,w,c', V.POOL_SHAPES)
def test_maxpool_selects_exactly(ops, B, h, w, c, dt):
    e = V.pool_case(B, h, w, c)
    xd, dyd = put(e.x, dt), put(e.dy, dt)
    y = gout((B, h // 2, w // 2, c), dt)
    ops.maxpool2_fwd(xd, y, B, h, w, c)
    torch.cuda.synchronize()
    yv = widen(y)
    assert np.isfinite(yv).all() and (yv == V.pool_fwd(e.x)).all(), 'the window maximum, as a number (+0 == -0)'
    for relu in (0, 1):
        dx = gout((B, h, w, c), dt)
        ops.maxpool2_bwd(xd, dyd, dx, B, h, w, c, relu)
        torch.cuda.synchronize()
        ref = V.pool_bwd(e.dy, e.x, relu)
        same(dx, ref, dt, 'maxpool2_bwd relu_mask=%d' % relu)
        _am, win = V.window_argmax(widen(dx))
        live = e.dy != 0
        if relu:
            live = live & (V.pool_fwd(e.x) > 0)
            dead = np.repeat(np.repeat(~(V.pool_fwd(e.x) > 0), 2, 1), 2, 2)
            assert (widen(dx)[dead] == 0).all(), 'no gradient into a window whose maximum is not > 0'
        assert ((win != 0).sum(3) == live).all(), 'exactly one non-zero per window and channel where the gradient counts'


# ==============================================================================================
# 2. resize, align corners
# ==============================================================================================
@DT
@pytest.mark.parametrize('hi,wi,ho,wo', V.RESIZE_EXACT)
def test_resize_exact(ops, hi, wi, ho, wo, dt):
    e = V.resize_exact_case(hi, wi, ho, wo, dt)
    B, c, ldx, ldy = V.RESIZE_EXACT_B, V.RESIZE_EXACT_C, V.RESIZE_EXACT_LDX, V.RESIZE_EXACT_LDY
    y = gout((B, ho, wo, ldy), dt)
    ops.resize_ac_fwd(put(e.x, dt, ldx), y, B, hi, wi, ho, wo, c, ldx, ldy)
    dx = gout((B, hi, wi, ldx), dt)
    ops.resize_ac_bwd(put(e.dy, dt, ldy), dx, B, hi, wi, ho, wo, c, ldy, ldx)
    torch.cuda.synchronize()
    same(y[..., :c], e.fwd.y, dt, 'resize_ac_fwd %dx%d -> %dx%d' % (hi, wi, ho, wo))
    same(dx[..., :c], e.bwd.dx, dt, 'resize_ac_bwd %dx%d <- %dx%d' % (hi, wi, ho, wo))
    assert untouched(y[..., c:]) and untouched(dx[..., c:])
    if dt == F32:                                                            # (a 16-bit store rounds: the identity is the exact values')
        assert float((widen(y[..., :c]) * e.dy).sum()) == float((e.x * widen(dx[..., :c])).sum()), '<resize(x), dy> == <x, resize_bwd(dy)>'


@DT
@pytest.mark.parametrize('B,hi,wi,ho,wo,c,ldx,ldy', V.RESIZE_BOUNDED)
def test_resize_within_bounds(ops, B, hi, wi, ho, wo, c, ldx, ldy, dt):
    e = V.resize_bounded_case(B, hi, wi, ho, wo, c, dt)
    y = gout((B, ho, wo, ldy), dt)
    ops.resize_ac_fwd(wide(e.x_t, ldx), y, B, hi, wi, ho, wo, c, ldx, ldy)
    dx = gout((B, hi, wi, ldx), dt)
    ops.resize_ac_bwd(wide(e.dy_t, ldy), dx, B, hi, wi, ho, wo, c, ldy, ldx)
    torch.cuda.synchronize()
    tag = '%dx%d -> %dx%d c%d %s' % (hi, wi, ho, wo, c, V.STORAGE_IDS[V.STORAGE.index(dt)])
    held(y[..., :c], e.fwd.y, e.fwd.bound, dt, 'resize_ac_fwd ' + tag)
    held(dx[..., :c], e.bwd.dx, e.bwd.bound, dt, 'resize_ac_bwd ' + tag)
    assert untouched(y[..., c:]) and untouched(dx[..., c:])


# ==============================================================================================
# 3. gray + conv1_1 forward
# ==============================================================================================
@DT
@pytest.mark.parametrize('s,B,ldp', V.FWD_CASES)
def test_vgg_conv1_1_fwd_within_bounds(ops, s, B, ldp, dt):
    im = V.images(B, s, ldp)
    gtd, pd = dev(im.gt), dev(im.pred)                                      # pred ends on its guard band; columns [3, ldp) hold NaN
    for kind in ('random', 'structured'):
        w9, b = V.bank(kind)
        wd, bd = dev(torch.from_numpy(w9)), dev(torch.from_numpy(b))
        r = V.cached(('conv1_1', B, s, ldp, kind), lambda: V.conv1_1(im.both, w9, b))
        out = gout((2 * B, s, s, 64), dt)
        ops.vgg_conv1_1_fwd(gtd, pd, ldp, B, s, wd, bd, out, 3)
        two = gout((2 * B, s, s, 64), dt)
        ops.vgg_conv1_1_fwd(gtd, pd, ldp, B, s, wd, bd, two, 1)
        torch.cuda.synchronize()
        held(out, r.a, r.bound, dt, 'vgg_conv1_1_fwd s%d B%d ldp%d %s %s' % (s, B, ldp, kind, V.STORAGE_IDS[V.STORAGE.index(dt)]))
        assert untouched(two[B:]), 'halves = 1 writes the gt images alone'
        assert torch.equal(bits(two[:B]), bits(out[:B]))
        ops.vgg_conv1_1_fwd(gtd, pd, ldp, B, s, wd, bd, two, 2)
        torch.cuda.synchronize()
        assert torch.equal(bits(two), bits(out)), 'halves 1 then 2 == halves 3, bit for bit'


# ==============================================================================================
# 4. conv1_1 backward: exact operands, two f32 roundings
# ==============================================================================================
@DT
@pytest.mark.parametrize('s,B,ld', V.BWD_CASES, ids=['s%d_B%d_ldp%d_lddp%d' % (s, B, ld[0], ld[1]) for s, B, ld in V.BWD_CASES])
def test_vgg_conv1_1_bwd_two_roundings(ops, s, B, ld, dt):
    """The pixel stride of dpred IS lddp, so 'past lddp' is the next pixel or, after the last one, the guard band."""
    ldp, lddp = ld
    e = V.bwd_case(B, s, ldp)
    dzd, wd = put(e.dz, dt), put(e.w, F32)
    gtd, pd, md = put(e.gt, F32), put(e.pred, F32, ldp), put(e.mask, F32)
    coefd = dev(torch.tensor(V.BWD_COEF))
    same_px = (e.pred == e.gt).all(-1)
    for mask_given, idx, l1 in V.BWD_PARAMS:
        dp = gout((B, s, s, lddp), dt)
        ops.vgg_conv1_1_bwd(dzd, B, s, wd, gtd, pd, ldp, md if mask_given else None, coefd, dp, lddp, input_idx=idx, l1=l1)
        torch.cuda.synchronize()
        r = V.conv1_1_bwd(e.dz, e.w, e.gt, e.pred, e.mask if mask_given else None, V.BWD_COEF[idx] if idx >= 0 else 0.0, l1)
        held(dp[..., :3], r.o, r.bound, dt, 'vgg_conv1_1_bwd s%d B%d lddp%d mask%d idx%d l1%d %s' % (
            s, B, lddp, mask_given, idx, l1, V.STORAGE_IDS[V.STORAGE.index(dt)]))
        assert bool((bits(dp[..., 3:]) == 0).all()), 'channels 3 .. lddp - 1 are +0'
        # where the direct term is 0 (pred == gt, or no direct term at all) the three channels ARE the convolution term: one value,
        # and (by the bound, which has no addition there) the f32 quotient itself
        flat = same_px if idx >= 0 else np.ones_like(same_px)
        got = bits(dp[..., :3]).cpu()[torch.from_numpy(flat)]
        assert bool((got == got[:, :1]).all()) and got.shape[0] > 0


# ==============================================================================================
# 5. the head in one launch
# ==============================================================================================
def run_head(ops, im, B, S, ldp, f, dt, store_from):
    from imm_amd import _lib as L
    assert ops.vgg_head_supported(B, S, dt)
    fd = ops.fwd_desc(2 * B, S, S, 64, 64, 64, 64, 3, 1, L.CONV_BIAS | L.CONV_RELU)
    wt = gout((128, fd.kpad), dt, fill=0)
    ops.pack_weights(dev(T64(f.w12).float()), wt, 0, 3, 3, 64, 64, 64, 128, fd.kpad)
    a11, y12 = gout((2 * B, S, S, 64), dt), gout((2 * B, S, S, 64), dt)
    scratch = gout((ops.vgg_head_scratch_bytes(B, S),), torch.uint8)
    ops.vgg_head_fwd(dev(im.gt), dev(im.pred), ldp, B, S, dev(torch.from_numpy(f.w11)), dev(torch.from_numpy(f.b11)), wt,
                     dev(T64(f.b12).float()), a11, store_from, y12, scratch)
    torch.cuda.synchronize()
    return a11, y12


HEAD_EXACT = [(1, 32, 3, 'one_patch_per_workgroup'), (1, 48, 8, 'grid_36_decode_not_pow2'), (None, 128, 3, 'five_patches_per_workgroup')]


@DT16
@pytest.mark.parametrize('B,S,ldp,tag', HEAD_EXACT, ids=[c[-1] for c in HEAD_EXACT])
def test_vgg_head_conv1_2_bit_for_bit(ops, B, S, ldp, tag, dt):
    big = B is None
    if big:
        cus = ops.device_info()[0]
        B = V.head_big_batch(cus, S)
        assert 2 * B * (S // 16) * (S // 8) >= 5 * cus
    f = V.head_exact_filters()
    im = V.images(B, S, ldp)
    a11, y12 = run_head(ops, im, B, S, ldp, f, dt, 0)
    a = a11.cpu().float().numpy()
    live = np.ones(64, bool)
    live[V.HEAD_DEAD] = False
    assert (a[..., ~live] == 0).all() and (a[..., live] >= 4).all() and (a[..., live] < 8).all(), 'the premise, on what was stored'
    if not big:
        ra = V.head_a11(im.both, f.w11, f.b11, dt)
        held(a11, ra.a, ra.bound, dt, 'vgg_head a11 (b11 = +-6) %s S%d %s' % (tag, S, V.SIXTEEN_IDS[V.SIXTEEN.index(dt)]))
    r = V.conv1_2(a, f.w12.astype(np.float32), f.b12.astype(np.float32), f32=True) if big else V.conv1_2(a, f.w12, f.b12)
    same(y12, r.y, dt, 'vgg_head y12 == RNE16(relu(conv(a11 as stored) + b12)) ' + tag)
    del r
    for sf in (B, 2 * B):
        a_sf, y_sf = run_head(ops, im, B, S, ldp, f, dt, sf)
        assert torch.equal(bits(y_sf), bits(y12)), 'store_from = %d changes y12' % sf
        assert untouched(a_sf[:sf]), 'images below store_from are not stored'
        assert torch.equal(bits(a_sf[sf:]), bits(a11[sf:]))


@DT16
@pytest.mark.parametrize('B,S,ldp', [(1, 32, 3), (1, 48, 8)])
def test_vgg_head_conv1_1_within_the_split_bound(ops, B, S, ldp, dt):
    f = V.head_real_filters(dt)
    im = V.images(B, S, ldp)
    a11, _y = run_head(ops, im, B, S, ldp, f, dt, 0)
    ra = V.head_a11(im.both, f.w11, f.b11, dt)
    held(a11, ra.a, ra.bound, dt, 'vgg_head a11 (real filters) S%d %s' % (S, V.SIXTEEN_IDS[V.SIXTEEN.index(dt)]))
    assert float((ra.a == 0).mean()) > 0.1 and float((ra.a > 0).mean()) > 0.1      # values at and near zero on both sides of the ReLU


@DT16
def test_vgg_head_real_data_against_f64(ops, dt):
    """y12 against f64 twice: from the conv1_1 activation the launch stored, taken as an operand (576 products, the matrix path, on
    values near zero), and from the images with the bound of conv1_1 carried through conv1_2."""
    B, S, ldp = 1, 32, 3
    f = V.head_real_filters(dt)
    im = V.images(B, S, ldp)
    a11, y12 = run_head(ops, im, B, S, ldp, f, dt, 0)
    name = V.SIXTEEN_IDS[V.SIXTEEN.index(dt)]
    ra = V.head_a11(im.both, f.w11, f.b11, dt)
    held(a11, ra.a, ra.bound, dt, 'vgg_head a11 (real data) ' + name)
    rs = V.conv1_2(widen(a11), f.w12, f.b12)
    held(y12, rs.y, V.y12_bound_from_stored(rs), dt, 'vgg_head y12 from the stored a11 ' + name)
    ri = V.conv1_2(ra.a, f.w12, f.b12)
    held(y12, ri.y, V.y12_bound_from_images(ra, ri, f.w12, dt), dt, 'vgg_head y12 from the images ' + name)
