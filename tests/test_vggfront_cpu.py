"""What tests/test_vggfront_gpu.py rests on, shown without a GPU (tests/vgg_reference.py).

A. The restatements are not copies of the kernels: the resize against oracle.resize_bilinear(align_corners=True) and its autograd, the
   pool against torch's max_pool2d, conv1_1 and its backward against the oracle's convolution and autograd.
B. The premises of the exact cases: every pool window kind is in the data; every resize weight and partial result is exact in f32, so
   contraction cannot matter; the conv1_1 backward's contraction is an integer and its direct term dyadic; the head's conv1_2 sums are
   exact in f32 under any order, its inputs lie in [4, 8) or are 0, and its outputs do round (the shares of tests/test_exact_cpu.py).
C. The f32 emulations of the bounded cases stay inside the bounds (worst err/bound printed: run with -s).
D. Each comparison can fail: a truncating store, ties rounded away, the whi glo term dropped, padding before normalisation, the pool
   gradient at the last maximum, half-pixel coordinates and a lerp taken from the 16-bit value are each rejected on the committed data.
E. The entry points refuse, before any launch: odd pool sides, lddp outside {8, .., 64 step 8}, a head side below 32 or no multiple
   of 16, store_from out of range.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from oracle import imm_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_data as E                                                      # noqa: E402
import vgg_reference as V                                                   # noqa: E402

DT = pytest.mark.parametrize('dt', V.STORAGE, ids=V.STORAGE_IDS)
DT16 = pytest.mark.parametrize('dt', V.SIXTEEN, ids=V.SIXTEEN_IDS)
quiet = lambda *_a: None                                                     # noqa: E731


def as_stored(v32, dt, how='rne'):
    """f32 values as the tensor of type dt a store leaves (how: rne, or the wrong trunc / away)."""
    return torch.from_numpy(V.rounded(v32, dt, how)).to(dt)


def rejected(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a, out=quiet) if fn is V.held else fn(*a)


# ==============================================================================================
# A. the restatements against the oracle
# ==============================================================================================
ALL_PAIRS = sorted(set(V.RESIZE_EXACT) | {c[1:5] for c in V.RESIZE_BOUNDED})


@pytest.mark.parametrize('hi,wi,ho,wo', ALL_PAIRS)
def test_resize_equals_the_oracle_and_its_autograd(hi, wi, ho, wo):
    g = np.random.RandomState(hi + wi + ho + wo)
    x, dy = g.standard_normal((2, hi, wi, 3)), g.standard_normal((2, ho, wo, 3))
    xt = V.T64(x).requires_grad_(True)
    yt = O.resize_bilinear(xt, ho, wo, align_corners=True)
    (gx,) = torch.autograd.grad(yt, xt, V.T64(dy))
    f, b = V.resize_fwd(x, ho, wo), V.resize_bwd(dy, hi, wi)
    # loose: the oracle's coordinates are f64, the kernel's f32; the lerp is continuous across a floor that falls differently
    assert np.abs(f.y - yt.detach().numpy()).max() < 1e-5 and np.abs(b.dx - gx.numpy()).max() < 1e-4
    # the matrix form (the adjoint's) is the lerp form, and the adjoint identity holds
    assert np.abs(np.einsum('Yi,bijc,Xj->bYXc', b.wy, x, b.wx) - f.y).max() < 1e-12
    assert abs((f.y * dy).sum() - (x * b.dx).sum()) < 1e-9
    assert np.isfinite(f.bound).all() and np.isfinite(b.bound).all()


@pytest.mark.parametrize('B,h,w,c', V.POOL_SHAPES)
def test_pool_equals_torch(B, h, w, c):
    e = V.pool_case(B, h, w, c)
    ref = torch.nn.functional.max_pool2d(V.T64(e.x).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).numpy()
    assert (V.pool_fwd(e.x) == ref).all()


def test_conv1_1_equals_the_oracle_and_autograd():
    im = V.images(2, 17, 5)
    w9, b = V.bank('random')
    r = V.conv1_1(im.both, w9, b)
    ims = V.T64(im.both)
    pr = ims[2:].clone().requires_grad_(True)
    gray = torch.cat([ims[:2], pr], 0).mean(dim=3, keepdim=True) / 255.0 - O.VGG_GRAY_MEAN / 255.0
    a = torch.relu(O.conv2d_same(gray, V.T64(w9).reshape(3, 3, 1, 64), V.T64(b)))
    assert np.abs(r.a - a.detach().numpy()).max() < 1e-12
    assert (r.bound > 0).all() and float(r.bound.max()) < 64 * V.U * float(r.terms.max())
    # backward: d/dpred of sum(dz z) + coef/2 sum(mask (pred - gt)^2) (l2) or coef sum(mask |pred - gt|) (l1)
    e = V.bwd_case(2, 17, 4)
    for l1 in (False, True):
        pr = V.T64(e.pred).requires_grad_(True)
        g = pr.mean(dim=3, keepdim=True) / 255.0 - O.VGG_GRAY_MEAN / 255.0
        z = O.conv2d_same(g, V.T64(e.w).reshape(3, 3, 1, 64), None)
        d = pr - V.T64(e.gt)
        direct = (V.T64(e.mask).unsqueeze(-1) * (d.abs() if l1 else 0.5 * d * d)).sum()
        (gp,) = torch.autograd.grad((z * V.T64(e.dz)).sum() + 0.375 * direct, pr)
        ref = V.conv1_1_bwd(e.dz, e.w, e.gt, e.pred, e.mask, 0.375, l1)
        assert np.abs(ref.o - gp.numpy()).max() < 1e-9


# ==============================================================================================
# B. premises of the exact cases
# ==============================================================================================
@pytest.mark.parametrize('B,h,w,c', V.POOL_SHAPES)
def test_pool_data_hold_every_window_kind(B, h, w, c):
    e = V.pool_case(B, h, w, c)
    for dt in V.STORAGE:
        assert torch.equal(V.store(e.x, dt).double(), V.T64(e.x)) and torch.equal(V.store(e.dy, dt).double(), V.T64(e.dy))
    am, wv = V.window_argmax(e.x)                                          # wv [B, h/2, w/2, 4, c]
    mx = wv.max(3)
    nmax = (wv == mx[:, :, :, None, :]).sum(3)
    for q in range(4):
        assert ((am == q) & (nmax == 1)).any(), 'no window with its unique maximum at position %d' % q
    hot = np.moveaxis(wv == mx[:, :, :, None, :], 3, -1).reshape(-1, 4)
    pos = np.moveaxis(wv, 3, -1).reshape(-1, 4)
    for i in range(4):
        for j in range(i + 1, 4):
            want = np.zeros(4, bool)
            want[[i, j]] = True
            assert ((hot == want).all(1) & (pos.max(1) > 0)).any(), 'no positive two-way tie at (%d, %d)' % (i, j)
    assert (hot.all(1) & (pos.max(1) > 0)).any(), 'no positive four-way tie'
    assert (pos.max(1) < 0).any() and ((pos.max(1) < 0) & (hot.sum(1) > 1)).any(), 'no all-negative window (with a tie)'
    assert (pos.max(1) == 0).any(), 'no window whose maximum is 0'
    sb = np.signbit(pos)
    mixed = (pos.max(1) == 0) & ((pos == 0) & sb).any(1) & ((pos == 0) & ~sb).any(1)
    assert mixed.any() and (mixed & sb[:, 0] & (pos[:, 0] == 0)).any() and (mixed & ~sb[:, 0] & (pos[:, 0] == 0)).any(), \
        'no window that mixes +0 and -0 with either sign first'
    assert float((nmax > 1).mean()) > 0.2, 'ties must be frequent'
    assert (e.dy == 0).any() and (e.dy != 0).mean() > 0.5 and not np.signbit(e.dy[e.dy == 0]).any()
    # the two tie rules differ on these data, with and without the ReLU mask
    for relu in (0, 1):
        assert (V.pool_bwd(e.dy, e.x, relu) != V.pool_bwd(e.dy, e.x, relu, last=True)).any()
    assert (V.pool_bwd(e.dy, e.x, 1) != V.pool_bwd(e.dy, e.x, 0)).any()


@DT
@pytest.mark.parametrize('hi,wi,ho,wo', V.RESIZE_EXACT)
def test_resize_exact_cases_are_exact_in_f32(hi, wi, ho, wo, dt):
    e = V.resize_exact_case(hi, wi, ho, wo, dt)
    assert torch.equal(V.store(e.x, dt).double(), V.T64(e.x)) and torch.equal(V.store(e.dy, dt).double(), V.T64(e.dy))
    for n_in, n_out in ((hi, ho), (wi, wo)):
        _lo, _hi, lerp, src = V.ac_coord(n_in, n_out)
        assert (lerp * 4 == np.round(lerp * 4)).all() and (src == np.arange(n_out) * ((n_in - 1) / max(n_out - 1, 1))).all()
    f, b = e.fwd, e.bwd
    # every partial result of the forward, in the kernel's order: exact, so a contracted multiply-add gives the same value
    for name in ('dt_', 'db_', 'pt', 'pb', 'top', 'bot', 'dv', 'pv', 'y'):
        assert V.exact_in_f32(getattr(f, name)), name
    assert (V.resize_fwd_f32(e.x, ho, wo).astype(np.float64) == f.y).all()
    # the adjoint: weights are multiples of 1/16, so every term is, and every partial sum stays below 2^24 of them
    for W in (b.wy, b.wx):
        assert (W * 4 == np.round(W * 4)).all() and V.exact_in_f32(W) and V.exact_in_f32(1.0 - W)
    assert float(b.terms.max()) * 16 < 2 ** 24 and (b.dx * 16 == np.round(b.dx * 16)).all()
    assert (f.y * e.dy).sum() == (e.x * b.dx).sum(), 'the integer adjoint identity'
    V.stored_bits(f.y, dt), V.stored_bits(b.dx, dt)                          # (asserts f32-exact and finite in dt)
    if dt != V.F32T and (hi - 1) % max(ho - 1, 1) and (wi - 1) % max(wo - 1, 1):
        for v in (f.y, b.dx):                                                # fractional weights along both axes: the store rounds
            n_inexact, _t, _o = E.rounding_mix(V.T64(v), dt)
            assert n_inexact > 0.2, (n_inexact, dt)


@pytest.mark.parametrize('s,B,ld', V.BWD_CASES)
def test_conv1_1_backward_operands_are_exact(s, B, ld):
    e = V.bwd_case(B, s, ld[0])
    for dt in V.STORAGE:
        assert torch.equal(V.store(e.dz, dt).double(), V.T64(e.dz)) and torch.equal(V.store(e.w, dt).double(), V.T64(e.w))
    assert 576 * 4 * 3 < 2 ** 24
    n_same = 0
    for mask_given, idx, l1 in V.BWD_PARAMS:
        r = V.conv1_1_bwd(e.dz, e.w, e.gt, e.pred, e.mask if mask_given else None, V.BWD_COEF[idx] if idx >= 0 else 0.0, l1)
        assert V.exact_in_f32(r.part) and V.exact_in_f32(r.direct) and (r.part == np.round(r.part)).all()
        assert (r.direct == 0).all() == (idx < 0)
        n_same += int(((e.pred == e.gt).all(-1)).sum())
        out = V.conv1_1_bwd_f32(e.dz, e.w, e.gt, e.pred, e.mask if mask_given else None, V.BWD_COEF[idx] if idx >= 0 else 0.0, l1)
        for dt in V.STORAGE:
            V.held(V.rounded(out, dt), r.o, r.bound, dt, 'bwd emulation', out=quiet)
    assert n_same > 0, 'pixels with pred == gt'


@DT16
def test_head_conv1_2_premise_and_rounding_shares(dt):
    f = V.head_exact_filters()
    im = V.images(1, 32, 3)
    a = V.rounded(V.head_a11_f32(im.both, f.w11, f.b11, dt), dt)
    live = np.ones(64, bool)
    live[V.HEAD_DEAD] = False
    assert (a[..., ~live] == 0).all() and (a[..., live] >= 4).all() and (a[..., live] < 8).all()
    grain = 2.0 ** (3 - V.PBITS[dt])                                         # the ulp of the type in [4, 8)
    assert (a / grain == np.round(a / grain)).all()
    assert (f.w12 == np.round(f.w12)).all() and np.abs(f.w12).max() <= 3 and (f.b12 * 2 == np.round(f.b12 * 2)).all()
    for v in (f.w12, ):
        assert torch.equal(V.store(v, dt).double(), V.T64(v))
    r = V.conv1_2(a, f.w12, f.b12)
    assert float(r.terms.max()) / min(grain, 0.5) < 2 ** 24, 'every partial sum, in any order, is exact in f32'
    assert (V.conv1_2(a, f.w12, f.b12, f32=True).z == r.z).all()
    # shuffled f32 summation of the 577 terms of a few outputs
    g = np.random.RandomState(5)
    ap = np.pad(a, ((0, 0), (1, 1), (1, 1), (0, 0)))
    for _ in range(40):
        n, y, x, co = g.randint(0, a.shape[0]), g.randint(0, 32), g.randint(0, 32), g.randint(0, 64)
        terms = np.concatenate([(ap[n, y:y + 3, x:x + 3, :] * f.w12[:, :, :, co]).reshape(-1), [f.b12[co]]]).astype(np.float32)
        for _k in range(3):
            acc = np.float32(0)
            for v in g.permutation(terms):
                acc = np.float32(acc + v)
            assert float(acc) == r.z[n, y, x, co]
    n_inexact, n_tie, n_other = E.rounding_mix(V.T64(r.y), dt)
    print('head y12 %s: %.1f %% not representable, %.1f %% ties, %.1f %% inexact non-ties' % (dt, 100 * n_inexact, 100 * n_tie, 100 * n_other))
    assert n_inexact >= 0.20 and n_tie >= 0.05 and n_other >= 0.05
    V.stored_bits(r.y, dt)
    # a halo of relu(b11) = 6 instead of 0 is off by far more than a rounding
    wrong = V.conv1_2(np.pad(a, ((0, 0), (1, 1), (1, 1), (0, 0)), constant_values=6.0), f.w12, f.b12).y[:, 1:-1, 1:-1]
    assert np.abs(wrong - r.y).max() > 16
    assert V.head_big_batch(256) == 5 and V.head_big_batch(304) == 6 and V.head_big_batch(8) == 1


# ==============================================================================================
# C. the f32 emulations stay inside the bounds
# ==============================================================================================
@DT
def test_emulations_within_bounds(dt):
    worst = {}
    for B, hi, wi, ho, wo, c, _ldx, _ldy in V.RESIZE_BOUNDED:
        e = V.resize_bounded_case(B, hi, wi, ho, wo, c, dt)
        y = V.resize_fwd_f32(e.x, ho, wo)
        worst['resize'] = max(worst.get('resize', 0), V.held(V.rounded(y, dt), e.fwd.y, e.fwd.bound, dt, 'resize emulation', out=quiet))
        assert float(e.fwd.bound.max()) < 1e-4 and float(e.bwd.bound.max()) < 1e-4
    for s, B, ldp in V.FWD_CASES[::5]:
        im = V.images(B, s, ldp)
        for kind in ('random', 'structured'):
            w9, b = V.bank(kind)
            r = V.conv1_1(im.both, w9, b)
            got = V.rounded(V.conv1_1_f32(im.both, w9, b), dt)
            worst[kind] = max(worst.get(kind, 0), V.held(got, r.a, r.bound, dt, 'conv1_1 emulation', out=quiet))
            if kind == 'structured':                                          # a handful of f32 ulps of the tap (|g| < 1)
                assert float((r.bound[..., :60] / np.abs(w9).max(0)[:60]).max()) < 20 * V.U and float(r.bound[..., 60:].max()) < 10 * V.U
    print('%s: worst err/bound of the f32 emulations %s' % (dt, {k: round(v, 3) for k, v in worst.items()}))


@DT16
@pytest.mark.parametrize('filters', ['exact', 'real'])
def test_head_split_emulation_within_bound(dt, filters):
    f = V.head_exact_filters() if filters == 'exact' else V.head_real_filters(dt)
    im = V.images(1, 32, 3)
    ra = V.head_a11(im.both, f.w11, f.b11, dt)
    got = V.head_a11_f32(im.both, f.w11, f.b11, dt)
    r32 = V.held(got, ra.a, ra.bound, V.F32T, 'head a11 emulation, unrounded', out=quiet)
    r16 = V.held(V.rounded(got, dt), ra.a, ra.bound, dt, 'head a11 emulation, stored', out=quiet)
    print('head a11 %s %s: worst err/bound %.3f before the store, %.3f stored; bound / |a| at most %.3g' % (
        dt, filters, r32, r16, float((ra.bound / np.maximum(ra.terms, 1e-30)).max())))
    # the split is the f32 product to 3 h^2: far below half an ulp of the storage type
    assert float((ra.bound / np.maximum(ra.terms, 1e-30)).max()) < 2.0 ** -V.PBITS[dt] / 8


# ==============================================================================================
# D. each comparison can fail
# ==============================================================================================
@pytest.mark.parametrize('B,h,w,c', V.POOL_SHAPES)
@pytest.mark.parametrize('relu', [0, 1])
def test_pool_gradient_at_the_last_maximum_is_rejected(B, h, w, c, relu):
    e = V.pool_case(B, h, w, c)
    for dt in V.STORAGE:
        V.same(V.store(V.pool_bwd(e.dy, e.x, relu), dt), V.pool_bwd(e.dy, e.x, relu), dt, 'pool')
        rejected(V.same, V.store(V.pool_bwd(e.dy, e.x, relu, last=True), dt), V.pool_bwd(e.dy, e.x, relu), dt, 'pool')


@DT16
def test_wrong_stores_are_rejected_by_the_exact_comparisons(dt):
    hi, wi, ho, wo = V.RESIZE_BOTH_FRACTIONAL[0]
    e = V.resize_exact_case(hi, wi, ho, wo, dt)
    y32 = V.resize_fwd_f32(e.x, ho, wo)
    V.same(as_stored(y32, dt), e.fwd.y, dt, 'resize')
    rejected(V.same, as_stored(y32, dt, 'trunc'), e.fwd.y, dt, 'resize')
    rejected(V.same, as_stored(y32, dt, 'away'), e.fwd.y, dt, 'resize')
    dx32 = e.bwd.dx.astype(np.float32)
    rejected(V.same, as_stored(dx32, dt, 'trunc'), e.bwd.dx, dt, 'resize_bwd')
    rejected(V.same, as_stored(dx32, dt, 'away'), e.bwd.dx, dt, 'resize_bwd')
    f = V.head_exact_filters()
    a = V.rounded(V.head_a11_f32(V.images(1, 32, 3).both, f.w11, f.b11, dt), dt)
    y = V.conv1_2(a, f.w12, f.b12).y
    V.same(as_stored(y.astype(np.float32), dt), y, dt, 'y12')
    rejected(V.same, as_stored(y.astype(np.float32), dt, 'trunc'), y, dt, 'y12')
    rejected(V.same, as_stored(y.astype(np.float32), dt, 'away'), y, dt, 'y12')


@DT16
def test_a_truncating_store_is_rejected_by_the_bounded_comparisons(dt):
    im = V.images(1, 17, 5)
    w9, b = V.bank('structured')
    r = V.conv1_1(im.both, w9, b)
    rejected(V.held, V.rounded(V.conv1_1_f32(im.both, w9, b), dt, 'trunc'), r.a, r.bound, dt, 'conv1_1')
    e = V.bwd_case(1, 17, 4)
    rb = V.conv1_1_bwd(e.dz, e.w, e.gt, e.pred, e.mask, 0.375, False)
    rejected(V.held, V.rounded(V.conv1_1_bwd_f32(e.dz, e.w, e.gt, e.pred, e.mask, 0.375, False), dt, 'trunc'), rb.o, rb.bound, dt, 'bwd')
    B, hi, wi, ho, wo, c, _x, _y = V.RESIZE_BOUNDED[0]
    eb = V.resize_bounded_case(B, hi, wi, ho, wo, c, dt)
    rejected(V.held, V.rounded(V.resize_fwd_f32(eb.x, ho, wo), dt, 'trunc'), eb.fwd.y, eb.fwd.bound, dt, 'resize')
    f = V.head_real_filters(dt)
    ra = V.head_a11(V.images(1, 32, 3).both, f.w11, f.b11, dt)
    rejected(V.held, V.rounded(V.head_a11_f32(V.images(1, 32, 3).both, f.w11, f.b11, dt), dt, 'trunc'), ra.a, ra.bound, dt, 'a11')


@DT16
@pytest.mark.parametrize('filters', ['exact', 'real'])
def test_the_dropped_hi_lo_term_is_rejected(dt, filters):
    f = V.head_exact_filters() if filters == 'exact' else V.head_real_filters(dt)
    im = V.images(1, 32, 3)
    ra = V.head_a11(im.both, f.w11, f.b11, dt)
    wrong = V.head_a11_f32(im.both, f.w11, f.b11, dt, drop='hi_lo')
    rejected(V.held, wrong, ra.a, ra.bound, V.F32T, 'a11 before the store')
    rejected(V.held, V.rounded(wrong, dt), ra.a, ra.bound, dt, 'a11 as stored')


@DT
@pytest.mark.parametrize('kind', ['random', 'structured'])
def test_padding_before_normalisation_is_rejected(dt, kind):
    im = V.images(1, 17, 5)
    w9, b = V.bank(kind)
    r = V.conv1_1(im.both, w9, b)
    wrong = V.conv1_1_f32(im.both, w9, b, pad_pixels=True)
    assert (wrong[:, 1:-1, 1:-1] == V.conv1_1_f32(im.both, w9, b)[:, 1:-1, 1:-1]).all()      # the interior cannot tell
    rejected(V.held, V.rounded(wrong, dt), r.a, r.bound, dt, 'conv1_1')
    assert np.abs(V.conv1_1(im.both, w9, b, pad_pixels=True).a - r.a).max() > 1e3 * float(r.bound.max())


@DT
def test_half_pixel_coordinates_and_a_16_bit_lerp_are_rejected(dt):
    for hi, wi, ho, wo in V.RESIZE_EXACT[:4]:
        e = V.resize_exact_case(hi, wi, ho, wo, dt)
        rejected(V.same, as_stored(V.resize_fwd_f32(e.x, ho, wo, coord=V.half_pixel_coord), dt), e.fwd.y, dt, 'resize')
        rejected(V.same, as_stored(V.resize_bwd(e.dy, hi, wi, coord=V.half_pixel_coord).dx.astype(np.float32), dt), e.bwd.dx, dt, 'resize_bwd')
    for B, hi, wi, ho, wo, c, _x, _y in V.RESIZE_BOUNDED:
        e = V.resize_bounded_case(B, hi, wi, ho, wo, c, dt)
        rejected(V.held, V.rounded(V.resize_fwd_f32(e.x, ho, wo, coord=V.half_pixel_coord), dt), e.fwd.y, e.fwd.bound, dt, 'resize')
        rejected(V.held, V.rounded(V.resize_bwd(e.dy, hi, wi, coord=V.half_pixel_coord).dx.astype(np.float32), dt), e.bwd.dx, e.bwd.bound, dt, 'bwd')
    for mid in V.SIXTEEN:
        if dt == V.F32T or mid == dt:
            # 5 -> 9 with 3 -> 9: the horizontal lerp has a fraction that the type loses; real data at every ratio
            for hi, wi, ho, wo in V.RESIZE_BOTH_FRACTIONAL:
                e = V.resize_exact_case(hi, wi, ho, wo, dt)
                rejected(V.same, as_stored(V.resize_fwd_f32(e.x, ho, wo, mid=mid), dt), e.fwd.y, dt, 'resize')
            for B, hi, wi, ho, wo, c, _x, _y in V.RESIZE_BOUNDED:
                e = V.resize_bounded_case(B, hi, wi, ho, wo, c, dt)
                rejected(V.held, V.rounded(V.resize_fwd_f32(e.x, ho, wo, mid=mid), dt), e.fwd.y, e.fwd.bound, dt, 'resize')


# ==============================================================================================
# E. refusals before any launch
# ==============================================================================================
def test_entry_points_refuse_before_any_launch():
    from imm_amd import _lib as L
    from imm_amd import ops
    lib = L.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                                                # non-null; never dereferenced: every call is refused
    bf, f32 = ops.dtype_enum(torch.bfloat16), ops.dtype_enum(torch.float32)
    for h, w in ((3, 4), (4, 3), (1, 1)):
        assert lib.imm_maxpool2_fwd(p, p, bf, 1, h, w, 8, None) == -1 and b'even sides' in lib.imm_last_error()
        assert lib.imm_maxpool2_bwd(p, p, p, f32, 1, h, w, 8, 0, None) == -1 and b'even sides' in lib.imm_last_error()
    assert lib.imm_maxpool2_fwd(p, p, bf, 1, 4, 4, 12, None) == -1
    for lddp in (0, 3, 12, 72):
        for dt in (bf, f32):
            assert lib.imm_vgg_conv1_1_bwd(p, dt, 1, 16, p, p, p, 3, None, p, 0, 0, p, lddp, None) == -1
            assert b'vgg_conv1_1_bwd' in lib.imm_last_error()
    assert lib.imm_vgg_conv1_1_bwd(p, bf, 1, 16, p, p, p, 2, None, p, 0, 0, p, 8, None) == -1            # ldp < 3
    assert lib.imm_vgg_conv1_1_fwd(p, p, 3, 1, 16, p, p, p, bf, 4, None) == -1 and b'halves' in lib.imm_last_error()
    assert lib.imm_resize_ac_fwd(p, p, bf, 1, 4, 4, 4, 4, 8, 4, 8, None) == -1                          # ldx < c
    assert lib.imm_resize_ac_bwd(p, p, bf, 1, 4, 4, 0, 4, 8, 8, 8, None) == -1                          # an empty output
    for s in (16, 24, 40, 0):
        assert not lib.imm_vgg_head_supported(1, s, bf)
        assert lib.imm_vgg_head_fwd(p, p, 3, 1, s, p, p, p, 576, p, p, 0, p, p, bf, None) == -1
        assert b'not served' in lib.imm_last_error()
    assert lib.imm_vgg_head_supported(1, 32, bf) and not lib.imm_vgg_head_supported(1, 32, f32)
    assert lib.imm_vgg_head_fwd(p, p, 3, 1, 32, p, p, p, 576, p, p, 0, p, p, f32, None) == -1
    for sf in (-1, 3):
        assert lib.imm_vgg_head_fwd(p, p, 3, 1, 32, p, p, p, 576, p, p, sf, p, p, bf, None) == -1
        assert b'store_from' in lib.imm_last_error()
    assert lib.imm_vgg_head_fwd(p, p, 3, 1, 32, p, p, p, 512, p, p, 0, p, p, bf, None) == -1           # the filter's row length
